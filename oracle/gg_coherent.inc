/*
 * gg_coherent.inc — CPU restatement of the coherent ("Mode C") path:
 * pr_l1_pr_l2_dram_directory_msi with the DRAM directory, DRAM controller,
 * ShmemPerfModel clock, memory network and lax-barrier quanta, driven in the
 * canonical schedule of DESIGN.md §Mode C.  Included by gg_oracle.c (one
 * translation unit: it reuses the cache, history-tree and NoC restatements).
 *
 * TEST INFRASTRUCTURE ONLY (see gg_oracle.h).
 *
 * Canonical schedule (the reference orders work by real-time thread arrival,
 * SURVEY.md §0 finding 3; this is one legal, deterministic order):
 *   quantum q (lax barrier at (q+1)*quantum, lax_barrier_sync_client.cc:31-69):
 *     step loop, until a step sends no message:
 *       every owned tile (independently):
 *         1. handles the messages delivered to it, per-channel FIFO (sender's
 *            sequence order), channels merged by (arrival time, sender);
 *         2. runs its trace while not blocked on a miss and the next access
 *            starts before the barrier;
 *       every message sent in the step is routed (NetworkModel) and delivered
 *       to the next step if sender and receiver share a logical shard, else
 *       held until the quantum boundary.
 *     boundary: held messages are delivered (exchanged between ranks).
 *   The L1 -> L2 request of a miss (a self message, l1_cache_cntlr.cc:169-170)
 *   is handled at once by the L2 (l2_cache_cntlr.cc:226-258); every other
 *   message goes through delivery, self-sends included (zero network time).
 */

/* ---- message types, components -------------------------------------------- */
enum { M_EX_REQ = GG_MSG_EX_REQ, M_SH_REQ = GG_MSG_SH_REQ, M_INV_REQ = GG_MSG_INV_REQ,
       M_FLUSH_REQ = GG_MSG_FLUSH_REQ, M_WB_REQ = GG_MSG_WB_REQ, M_EX_REP = GG_MSG_EX_REP,
       M_SH_REP = GG_MSG_SH_REP, M_INV_REP = GG_MSG_INV_REP, M_FLUSH_REP = GG_MSG_FLUSH_REP,
       M_WB_REP = GG_MSG_WB_REP, M_NULLIFY_REQ = GG_MSG_NULLIFY_REQ };

static int msg_to_directory(uint32_t t)   /* receiver DRAM_DIRECTORY vs L2_CACHE (memory_manager.cc:250-292) */
{
  return t == M_EX_REQ || t == M_SH_REQ || t == M_INV_REP || t == M_FLUSH_REP || t == M_WB_REP;
}
static int msg_has_data(uint32_t t)       /* ShmemMsg::getModeledLength (shmem_msg.cc:100-125) */
{
  return t == M_EX_REP || t == M_SH_REP || t == M_FLUSH_REP || t == M_WB_REP ||
         t == GG_MSG_DRAM_STORE_REQ || t == GG_MSG_DRAM_FETCH_REP ||  /* …sh_l2_msi/shmem_msg.cc:128-140 */
         t == GG_MSG_SH_REP_EX;   /* (MESI's DOWNGRADE_REP carries no data buffer: request length) */
}

/* DirectoryState::Type (directory_schemes/directory_state.h) */
enum { DS_UNCACHED = 0, DS_SHARED = 1, DS_MODIFIED = 2 };

#define C_INVALID_ADDR (~0ull)            /* INVALID_ADDRESS */
#define C_INVALID_TILE (-1)

/* DirectoryEntryFullMap (directory_entry_full_map.cc) + DirectoryEntry + DirectoryBlockInfo */
typedef struct {
  uint64_t addr;
  int32_t owner;
  uint32_t dstate;
  uint64_t* sharers;    /* BitVector over application tiles */
  uint64_t rng;         /* MOSI: the entry's Random<int> (drand48_r state X, 48 bits) */
} c_dentry;

/* ShmemReq (shmem_req.cc) queued in the per-address HashMapList (dram_directory_cntlr.h:46) */
typedef struct {
  uint64_t addr, time;        /* MSI: ShmemReq::_time; MOSI: _processing_finish_time (getTime) */
  uint32_t type, requester;
  /* MOSI ShmemReq (…mosi/shmem_req.h:14-66) */
  uint64_t arrival, start;    /* _arrival_time, _processing_start_time */
  uint32_t init_ds;           /* _initial_dstate */
  int32_t sharer;             /* _sharer_tile_id */
  int upgrade;                /* _upgrade_reply */
} c_req;

typedef struct {
  o_tile c;                   /* L1-D + L2 (the Mode-P restatement's pair) */
  /* application (the synthetic_memory-style core loop, synthetic_memory.cc:150-230) */
  uint64_t rec, rec_end;      /* next record, end of the tile's records */
  uint64_t clk;               /* core clock (ps) */
  int blocked;
  uint64_t pend_start;        /* initial time of the access waiting for its reply */
  /* L2CacheCntlr::_outstanding_shmem_msg (l2_cache_cntlr.h:64-66) */
  uint64_t out_addr, out_time;
  uint32_t seq;               /* next per-sender sequence number */
  /* directory slice (DirectoryCache, directory_cache.cc) */
  c_dentry** slot;            /* [sets * assoc] */
  c_dentry** replaced;        /* _replaced_directory_entry_list */
  uint32_t nreplaced, capreplaced;
  c_req** q;                  /* pending ShmemReqs in arrival order (per-address FIFO) */
  uint32_t nq, capq;
  /* DramPerfModel (dram_perf_model.cc) */
  oracle_htree* dram_q;
  /* inbox */
  gg_cmsg* in; uint64_t nin, capin;
  uint64_t st[GG_NUM_TILE_STATS];
  /* MOSI: DramDirectoryCntlr::_cached_data_list (addresses whose line the
   * directory holds, …mosi/dram_directory_cntlr.h:30-44) and the event counters */
  uint64_t* cdl; uint32_t ncdl, capcdl;
  uint64_t ps[GG_NUM_PROTO_STATS];
  /* pr_l1_sh_l2_msi: c.l2 is the tile's shared L2 slice; each of its lines
   * carries a directory entry (ShL2CacheLineInfo, …sh_l2_msi/cache_line_info.h),
   * and L2CacheCntlr::_evicted_cache_line_map holds evicted lines whose
   * sharers are being nullified (l2_cache_cntlr.h:60-62) */
  c_dentry** sde;             /* [sets * ways] */
  uint64_t* eva; o_line* evl; c_dentry** evd; uint32_t nev, capev;
} c_tile;

struct oracle_coh {
  gg_config cfg;
  uint32_t T, K, k0, k1;
  c_tile* t;
  /* derived constants */
  uint64_t lat_l1_data, lat_l1_tags, lat_l2_data, lat_l2_tags, lat_dir, gap_ps, quantum_ps;
  uint32_t log_line, dir_sets, dir_assoc, log_dir_sets, log_slices, sharer_words, bits_req, bits_data, bits_ifc;
  int mosi;                   /* cfg.protocol == GG_PROTO_MOSI */
  int shl2;                   /* cfg.protocol == GG_PROTO_SHL2_MSI or _MESI */
  int mesi;                   /* cfg.protocol == GG_PROTO_SHL2_MESI */
  uint32_t log_l2_sets;       /* sh_l2: L2CacheHashFn::_log_num_sets */
  uint64_t dram_proc, dram_cost;
  /* network */
  oracle_noc* noc;
  /* trace */
  const uint64_t* addr; const uint32_t* meta; uint64_t* out;
  /* messages */
  gg_cmsg* step; uint64_t nstep, capstep;           /* sent in the current step */
  /* tile-parallel steps (oracle_coh_set_threads): messages sent by the other
   * threads of a step go to their own buffers [1, nthreads); the batch is
   * sorted by (send time, sender, sequence) before routing, so the split is
   * invisible in every result */
  int nthreads;
  gg_cmsg** tstep; uint64_t* tnstep; uint64_t* tcapstep;
  gg_cmsg* bnd; uint64_t nbnd, capbnd;              /* held for the quantum boundary */
  gg_cmsg* res; uint64_t nres, capres;              /* held packets resuming in the next step */
  uint32_t* shard;                                  /* tile -> logical shard */
  uint64_t ri[GG_NUM_RUN_INFO];
  int err;
  int has_barrier, in_run;   /* BARRIER records in the trace; released by oracle_coh_run only */
  /* oracle_coh_set_quantum_hook: called by oracle_coh_run when quantum q has
   * ended and quantum nq runs next (nq = q + 1 after the last) */
  void (*qhook)(void* arg, uint64_t q, uint64_t nq);
  void* qhook_arg;
};
#define C_BAR_WAIT 2         /* c_tile.blocked of a tile waiting at a BARRIER record */

static uint32_t c_shard(const oracle_coh* C, uint32_t tile) { return C->shard[tile]; }
static int c_owned(const oracle_coh* C, uint32_t tile) { uint32_t s = c_shard(C, tile); return s >= C->k0 && s < C->k1; }

/* Logical shards = the reference's process -> tile mapping for
 * emesh_hop_by_hop with K processes (NetworkModelEMeshHopByHop::
 * computeProcessToTileMapping, network_model_emesh_hop_by_hop.cc:367-433):
 * 2-D blocks of the W x H mesh (W = floor(sqrt T), hop_by_hop.cc:55-59), so
 * an XY route between two tiles of one shard never leaves it.  Tile counts
 * that are not a full mesh: contiguous tile ranges. */
int oracle_shard_map(uint32_t T, uint32_t K, uint32_t* out)
{
  if (K == 0 || K > T) return GG_ERR_INVALID;
  const int W = (int)floor(sqrt((double)T)), H = (int)ceil(1.0 * T / W);
  if ((uint32_t)(W * H) != T) {
    for (uint32_t t = 0; t < T; ++t) out[t] = (uint32_t)(((uint64_t)t * K) / T);
    return 0;
  }
  for (uint32_t t = 0; t < T; ++t) out[t] = ~0u;
  const int pw = (int)floor(sqrt((double)K));
  const int ph = (int)floor(1.0 * K / pw);
  const int mhl = (int)((1.0 * H * pw * ph) / K);
  for (int i = 0; i < pw; ++i)
    for (int j = 0; j < ph; ++j) {
      int sx = W / pw, sy = mhl / ph;
      const int bx = i * sx, by = j * sy;
      if (i == pw - 1) sx = W - (pw - 1) * sx;
      if (j == ph - 1) sy = mhl - (ph - 1) * sy;
      for (int ii = 0; ii < sx; ++ii)
        for (int jj = 0; jj < sy; ++jj) out[(bx + ii) + (by + jj) * W] = (uint32_t)(i + j * pw);
    }
  const int left = (int)K - pw * ph;
  for (int i = pw * ph; i < (int)K; ++i) {
    int sx = W / left;
    const int sy = H - mhl, bx = (i - pw * ph) * sx, by = mhl;
    if (i == (int)K - 1) sx = W - (left - 1) * sx;
    for (int ii = 0; ii < sx; ++ii)
      for (int jj = 0; jj < sy; ++jj) out[(bx + ii) + (by + jj) * W] = (uint32_t)i;
  }
  uint32_t* seen = (uint32_t*)calloc(K, sizeof(uint32_t));
  int bad = 0;
  for (uint32_t t = 0; t < T; ++t) { if (out[t] >= K) bad = 1; else seen[out[t]] = 1; }
  for (uint32_t k = 0; k < K; ++k) if (!seen[k]) bad = 1;
  free(seen);
  return bad ? GG_ERR_INVALID : 0;
}

static void* grow(void* p, uint64_t* cap, uint64_t need, size_t el)
{
  if (need <= *cap) return p;
  uint64_t c = *cap ? *cap : 16;
  while (c < need) c *= 2;
  *cap = c;
  return realloc(p, c * el);
}

/* ---- DirectoryEntryFullMap ------------------------------------------------ */
static c_dentry* de_new(oracle_coh* C)          /* DirectoryEntry::create (directory_entry.cc:43-64) */
{
  c_dentry* e = (c_dentry*)calloc(1, sizeof(c_dentry));
  e->addr = C_INVALID_ADDR; e->owner = C_INVALID_TILE; e->dstate = DS_UNCACHED;
  e->sharers = (uint64_t*)calloc(C->sharer_words, sizeof(uint64_t));
  /* Random(): seed(time(NULL)) -> srand48_r (misc/random.h:14-23): X = seed << 16 | 0x330E */
  e->rng = ((uint64_t)(uint32_t)GG_MOSI_RNG_SEED << 16) | 0x330Eu;
  return e;
}
static void de_free(c_dentry* e) { if (e) { free(e->sharers); free(e); } }
static int de_has(const c_dentry* e, uint32_t s) { return (int)((e->sharers[s >> 6] >> (s & 63)) & 1); }
static uint32_t de_num(const oracle_coh* C, const c_dentry* e)
{
  uint32_t n = 0;
  for (uint32_t i = 0; i < C->sharer_words; ++i) n += (uint32_t)__builtin_popcountll(e->sharers[i]);
  return n;
}
static void de_add(oracle_coh* C, c_dentry* e, uint32_t s)   /* addSharer: LOG_ASSERT_ERROR(!at) (:27-33) */
{
  if (de_has(e, s)) C->err = 1;
  e->sharers[s >> 6] |= 1ull << (s & 63);
}
static void de_remove(oracle_coh* C, c_dentry* e, uint32_t s) /* removeSharer: assert(at) (:35-41) */
{
  if (!de_has(e, s)) C->err = 1;
  e->sharers[s >> 6] &= ~(1ull << (s & 63));
}
static void de_set_owner(oracle_coh* C, c_dentry* e, int32_t o)  /* DirectoryEntry::setOwner (directory_entry.cc:108-113) */
{
  if (o != C_INVALID_TILE && !de_has(e, (uint32_t)o)) C->err = 1;
  e->owner = o;
}

/* ---- DirectoryCache ------------------------------------------------------- */
/* The DirectoryCache constructor creates every entry (directory_cache.cc:60-72);
 * a fresh entry is INVALID_ADDRESS / UNCACHED / no sharers, so here it is
 * created on its slot's first use (67 M entries at 4096 tiles). */
static c_dentry* dc_slot(oracle_coh* C, c_tile* H, size_t i)
{
  if (!H->slot[i]) H->slot[i] = de_new(C);
  return H->slot[i];
}
/* computeSetIndex (directory_cache.cc:332-348): XOR of log2(sets)-bit chunks */
static uint32_t dc_set(const oracle_coh* C, uint64_t addr)
{
  uint64_t set = 0;
  for (uint32_t i = C->log_line + C->log_slices; (i + C->log_dir_sets) <= 64; i += C->log_dir_sets) {
    uint32_t bits = C->log_dir_sets;
    uint64_t mask = (bits >= 64) ? ~0ull : ((1ull << bits) - 1);
    set ^= (addr >> i) & mask;                   /* getBits<IntPtr>(address, i + log_sets, i) */
  }
  return (uint32_t)set;
}

/* getDirectoryEntry (directory_cache.cc:102-145); *t is the tile's ShmemPerfModel clock */
static c_dentry* dc_get(oracle_coh* C, c_tile* H, uint64_t addr, uint64_t* t)
{
  *t += C->lat_dir;                              /* enabled: incrCurrTime(_directory_access_latency) */
  H->st[GG_CT_DIR_ACCESSES]++;                   /* updateCounters */
  uint32_t set = dc_set(C, addr);
  for (uint32_t i = 0; i < C->dir_assoc; ++i) {
    c_dentry* e = dc_slot(C, H, (size_t)set * C->dir_assoc + i);
    if (e->addr == addr) return e;               /* + Latency(getLatency() = 0) */
  }
  for (uint32_t i = 0; i < C->dir_assoc; ++i) {
    c_dentry* e = dc_slot(C, H, (size_t)set * C->dir_assoc + i);
    if (e->addr == C_INVALID_ADDR) { e->addr = addr; return e; }
  }
  for (uint32_t i = 0; i < H->nreplaced; ++i)
    if (H->replaced[i]->addr == addr) return H->replaced[i];
  return NULL;
}

/* replaceDirectoryEntry (directory_cache.cc:163-213) */
static c_dentry* dc_replace(oracle_coh* C, c_tile* H, uint64_t replaced_addr, uint64_t addr, uint64_t* t)
{
  uint32_t set = dc_set(C, replaced_addr);
  c_dentry* ne = de_new(C);
  ne->addr = addr;
  c_dentry* old = NULL;
  for (uint32_t i = 0; i < C->dir_assoc; ++i) {
    c_dentry** s = &H->slot[(size_t)set * C->dir_assoc + i];
    if (!*s) *s = de_new(C);
    if ((*s)->addr == replaced_addr) { old = *s; *s = ne; break; }
  }
  if (!old) { C->err = 1; de_free(ne); return NULL; }
  if (H->nreplaced == H->capreplaced) {
    H->capreplaced = H->capreplaced ? 2 * H->capreplaced : 8;
    H->replaced = (c_dentry**)realloc(H->replaced, sizeof(c_dentry*) * H->capreplaced);
  }
  H->replaced[H->nreplaced++] = old;
  *t += C->lat_dir;
  H->st[GG_CT_DIR_ACCESSES]++;
  H->st[GG_CT_DIR_EVICTIONS]++;
  if (old->dstate != DS_UNCACHED) H->st[GG_CT_DIR_BACK_INVALIDATIONS]++;
  return ne;
}

/* invalidateDirectoryEntry (directory_cache.cc:215-231) */
static void dc_invalidate(oracle_coh* C, c_tile* H, uint64_t addr)
{
  for (uint32_t i = 0; i < H->nreplaced; ++i) {
    if (H->replaced[i]->addr == addr) {
      de_free(H->replaced[i]);
      memmove(&H->replaced[i], &H->replaced[i + 1], sizeof(c_dentry*) * (H->nreplaced - i - 1));
      H->nreplaced--;
      return;
    }
  }
  C->err = 1;
}

/* ---- the per-address request queue (HashMapList, misc/hash_map_list.h) ----
 * Requests live on the heap (a ShmemReq* each, as in the reference), so a
 * request stays where it is while others are queued or retired. */
static uint32_t rq_count(const c_tile* H, uint64_t addr)
{
  uint32_t n = 0;
  for (uint32_t i = 0; i < H->nq; ++i) n += (H->q[i]->addr == addr);
  return n;
}
static c_req* rq_front(c_tile* H, uint64_t addr)
{
  for (uint32_t i = 0; i < H->nq; ++i) if (H->q[i]->addr == addr) return H->q[i];
  return NULL;
}
static c_req* rq_enqueue(c_tile* H, c_req r)
{
  if (H->nq == H->capq) { H->capq = H->capq ? 2 * H->capq : 16; H->q = (c_req**)realloc(H->q, sizeof(c_req*) * H->capq); }
  c_req* p = (c_req*)malloc(sizeof(c_req));
  *p = r;
  H->q[H->nq++] = p;
  return p;
}
static void rq_dequeue(c_tile* H, uint64_t addr)
{
  for (uint32_t i = 0; i < H->nq; ++i) {
    if (H->q[i]->addr == addr) {
      free(H->q[i]);
      memmove(&H->q[i], &H->q[i + 1], sizeof(c_req*) * (H->nq - i - 1));
      H->nq--;
      return;
    }
  }
}

/* ---- MemoryManager::sendMsg (…msi/memory_manager.cc:306-332) -------------- */
static void c_send_rx(oracle_coh* C, uint32_t src, uint32_t dst, uint32_t type, uint32_t requester,
                      uint64_t addr, uint64_t time, uint32_t single_rx)
{
  c_tile* S = &C->t[src];
  gg_cmsg* m;
  const int tid = C->nthreads > 1 ? omp_get_thread_num() : 0;
  if (tid == 0) {
    C->step = (gg_cmsg*)grow(C->step, &C->capstep, C->nstep + 1, sizeof(gg_cmsg));
    m = &C->step[C->nstep++];
  } else {
    C->tstep[tid] = (gg_cmsg*)grow(C->tstep[tid], &C->tcapstep[tid], C->tnstep[tid] + 1, sizeof(gg_cmsg));
    m = &C->tstep[tid][C->tnstep[tid]++];
  }
  memset(m, 0, sizeof(*m));
  m->addr = addr; m->send_ps = time; m->arrival_ps = time;
  m->src = src; m->dst = dst; m->requester = requester; m->seq = S->seq++; m->type = type;
  m->hop = GG_HOP_NONE; m->single_rx = single_rx;
  S->st[GG_CT_MSGS_SENT]++;
  if (type == GG_MSG_INV_FLUSH_COMBINED_REQ) S->st[GG_CT_SENT_INV_FLUSH_COMBINED]++;
  else if (type >= GG_MSG_DRAM_FETCH_REQ && type <= GG_MSG_DRAM_FETCH_REP)
    S->st[GG_CT_SENT_DRAM_FETCH_REQ + type - GG_MSG_DRAM_FETCH_REQ]++;
  else if (type >= GG_MSG_DOWNGRADE_REQ) {}                   /* MESI's own types: msgs_sent only */
  else S->st[GG_CT_SENT_BY_TYPE + type - 1]++;
}
static void c_send(oracle_coh* C, uint32_t src, uint32_t dst, uint32_t type, uint32_t requester,
                   uint64_t addr, uint64_t time)
{
  c_send_rx(C, src, dst, type, requester, addr, time, 0);
}

/* AddressHomeLookup::getHome (address_home_lookup.cc:19-26): every tile has a controller */
static uint32_t c_home(const oracle_coh* C, uint64_t addr) { return (uint32_t)((addr >> 6) % C->T); }

/* ---- DramCntlr + DramPerfModel (dram_cntlr.cc:37-74, dram_perf_model.cc:75-116) */
static uint64_t dram_latency_ps(oracle_coh* C, c_tile* H, uint64_t t)
{
  uint64_t pkt_time_ns = (uint64_t)ceil(t / 1000.0);
  uint64_t qd = 0;
  if (H->dram_q) {
    qd = oracle_htree_delay(H->dram_q, pkt_time_ns, C->dram_proc);
    H->st[GG_CT_DRAM_QUEUE_REQUESTS]++;
  }
  uint64_t lat = qd + C->dram_proc + C->dram_cost;
  H->st[GG_CT_DRAM_ACCESSES]++;
  H->st[GG_CT_DRAM_LATENCY_NS] += lat;
  H->st[GG_CT_DRAM_QUEUE_DELAY_NS] += qd;
  return lat_to_ps(lat, 1.0);                    /* Latency(access_latency, DRAM_FREQUENCY = 1.0) */
}
static void dram_get(oracle_coh* C, c_tile* H, uint64_t* t) { *t += dram_latency_ps(C, H, *t); }
static void dram_put(oracle_coh* C, c_tile* H, uint64_t t) { (void)dram_latency_ps(C, H, t); }

/* ---- DramDirectoryCntlr (dram_directory_cntlr.cc) ------------------------- */
static void dd_process_ex(oracle_coh* C, uint32_t home, c_req* req, int cached, uint64_t* t);
static void dd_process_sh(oracle_coh* C, uint32_t home, c_req* req, int cached, uint64_t* t);

/* retrieveDataAndSendToL2Cache (:382-408) */
static void dd_retrieve_and_send(oracle_coh* C, uint32_t home, uint32_t type, uint32_t receiver,
                                 uint64_t addr, int cached, uint64_t* t)
{
  if (!cached) dram_get(C, &C->t[home], t);
  c_send(C, home, receiver, type, receiver, addr, *t);
}

static void dd_process_next(oracle_coh* C, uint32_t home, uint64_t addr, uint64_t* t);

/* processNullifyReq (:172-236) */
static void dd_process_nullify(oracle_coh* C, uint32_t home, c_req* req, uint64_t* t)
{
  c_tile* H = &C->t[home];
  uint64_t addr = req->addr;
  uint32_t requester = req->requester;
  c_dentry* e = dc_get(C, H, addr, t);
  if (!e) { C->err = 1; return; }
  switch (e->dstate) {
  case DS_MODIFIED:
    c_send(C, home, (uint32_t)e->owner, M_FLUSH_REQ, requester, addr, *t);
    break;
  case DS_SHARED:
    for (uint32_t s = 0; s < C->T; ++s)          /* getSharersList: ascending (directory_entry_full_map.cc:48-66) */
      if (de_has(e, s)) c_send(C, home, s, M_INV_REQ, requester, addr, *t);
    break;
  case DS_UNCACHED:
    dc_invalidate(C, H, addr);
    dd_process_next(C, home, addr, t);
    break;
  default: C->err = 1;
  }
}

/* processDirectoryEntryAllocationReq (:126-170) */
static c_dentry* dd_allocate(oracle_coh* C, uint32_t home, c_req* req, uint64_t* t)
{
  c_tile* H = &C->t[home];
  uint64_t addr = req->addr;
  uint32_t requester = req->requester;
  uint64_t msg_time = *t;
  /* getReplacementCandidates (directory_cache.cc:147-161): the assert's
   * getDirectoryEntry(address) runs in the reference build (no NDEBUG) */
  if (dc_get(C, H, addr, t) != NULL) C->err = 1;
  uint32_t set = dc_set(C, addr);
  c_dentry* cand = NULL;
  for (uint32_t i = 0; i < C->dir_assoc; ++i) {
    c_dentry* it = dc_slot(C, H, (size_t)set * C->dir_assoc + i);
    if ((cand == NULL || de_num(C, cand) > de_num(C, it)) && rq_count(H, it->addr) == 0) cand = it;
  }
  if (!cand) { C->err = 1; return NULL; }        /* "Cant find a directory entry to be replaced" */
  uint64_t replaced_addr = cand->addr;
  c_dentry* e = dc_replace(C, H, replaced_addr, addr, t);
  c_req nr = { replaced_addr, msg_time, M_NULLIFY_REQ, requester, 0, 0, 0, 0, 0 };
  rq_enqueue(H, nr);
  if (rq_count(H, replaced_addr) != 1) C->err = 1;
  dd_process_nullify(C, home, rq_front(H, replaced_addr), t);
  return e;
}

/* processExReqFromL2Cache (:238-312) */
static void dd_process_ex(oracle_coh* C, uint32_t home, c_req* req, int cached, uint64_t* t)
{
  c_tile* H = &C->t[home];
  uint64_t addr = req->addr;
  uint32_t requester = req->requester;
  c_dentry* e = dc_get(C, H, addr, t);
  if (!e) { c_req r = *req; e = dd_allocate(C, home, &r, t); if (!e) return; }
  switch (e->dstate) {
  case DS_MODIFIED:
    if (cached) C->err = 1;
    c_send(C, home, (uint32_t)e->owner, M_FLUSH_REQ, requester, addr, *t);
    break;
  case DS_SHARED:
    if (cached) C->err = 1;
    for (uint32_t s = 0; s < C->T; ++s)
      if (de_has(e, s)) c_send(C, home, s, M_INV_REQ, requester, addr, *t);
    break;
  case DS_UNCACHED:
    de_add(C, e, requester);
    de_set_owner(C, e, (int32_t)requester);
    e->dstate = DS_MODIFIED;
    dd_retrieve_and_send(C, home, M_EX_REP, requester, addr, cached, t);
    dd_process_next(C, home, addr, t);
    break;
  default: C->err = 1;
  }
}

/* processShReqFromL2Cache (:314-380) */
static void dd_process_sh(oracle_coh* C, uint32_t home, c_req* req, int cached, uint64_t* t)
{
  c_tile* H = &C->t[home];
  uint64_t addr = req->addr;
  uint32_t requester = req->requester;
  c_dentry* e = dc_get(C, H, addr, t);
  if (!e) { c_req r = *req; e = dd_allocate(C, home, &r, t); if (!e) return; }
  switch (e->dstate) {
  case DS_MODIFIED:
    if (cached) C->err = 1;
    c_send(C, home, (uint32_t)e->owner, M_WB_REQ, requester, addr, *t);
    break;
  case DS_SHARED:                                /* full map: addSharer always succeeds */
    de_add(C, e, requester);
    dd_retrieve_and_send(C, home, M_SH_REP, requester, addr, cached, t);
    dd_process_next(C, home, addr, t);
    break;
  case DS_UNCACHED:
    de_add(C, e, requester);
    e->dstate = DS_SHARED;
    dd_retrieve_and_send(C, home, M_SH_REP, requester, addr, cached, t);
    dd_process_next(C, home, addr, t);
    break;
  default: C->err = 1;
  }
}

/* dispatch the queue front after a time update (shared by :107-122, :427-455, :473-498, :523-538) */
static void dd_front_update_time(c_req* r, uint64_t* t)
{
  if (r->time < *t) r->time = *t;                /* ShmemReq::updateTime */
  if (*t < r->time) *t = r->time;                /* ShmemPerfModel::updateCurrTime */
}

/* processNextReqFromL2Cache (:98-124) */
static void dd_process_next(oracle_coh* C, uint32_t home, uint64_t addr, uint64_t* t)
{
  c_tile* H = &C->t[home];
  if (rq_count(H, addr) < 1) { C->err = 1; return; }
  rq_dequeue(H, addr);
  c_req* r = rq_front(H, addr);
  if (r) {
    dd_front_update_time(r, t);
    if (r->type == M_EX_REQ) dd_process_ex(C, home, r, 0, t);
    else if (r->type == M_SH_REQ) dd_process_sh(C, home, r, 0, t);
    else C->err = 1;
  }
}

/* handleMsgFromL2Cache (:43-96) and the INV/FLUSH/WB replies (:410-543) */
static void dd_handle(oracle_coh* C, uint32_t home, const gg_cmsg* m)
{
  c_tile* H = &C->t[home];
  uint64_t t = m->arrival_ps;                    /* MemoryManager::__handleMsgFromNetwork: setCurrTime(packet.time) */
  uint64_t addr = m->addr;
  uint32_t sender = m->src;
  switch (m->type) {
  case M_EX_REQ:
  case M_SH_REQ: {
    c_req r = { addr, t, m->type, m->requester, 0, 0, 0, 0, 0 };
    rq_enqueue(H, r);
    if (rq_count(H, addr) == 1) {
      c_req* f = rq_front(H, addr);
      if (m->type == M_EX_REQ) dd_process_ex(C, home, f, 0, &t);
      else dd_process_sh(C, home, f, 0, &t);
    }
    break;
  }
  case M_INV_REP: {                              /* processInvRepFromL2Cache (:410-456) */
    c_dentry* e = dc_get(C, H, addr, &t);
    if (!e || e->dstate != DS_SHARED) { C->err = 1; return; }
    de_remove(C, e, sender);
    if (de_num(C, e) == 0) e->dstate = DS_UNCACHED;
    if (rq_count(H, addr) > 0) {
      c_req* r = rq_front(H, addr);
      dd_front_update_time(r, &t);
      if (r->type == M_EX_REQ) { if (e->dstate == DS_UNCACHED) dd_process_ex(C, home, r, 0, &t); }
      else if (r->type == M_SH_REQ) dd_process_sh(C, home, r, 0, &t);
      else { if (e->dstate == DS_UNCACHED) dd_process_nullify(C, home, r, &t); }
    }
    break;
  }
  case M_FLUSH_REP: {                            /* processFlushRepFromL2Cache (:458-505) */
    c_dentry* e = dc_get(C, H, addr, &t);
    if (!e || e->dstate != DS_MODIFIED) { C->err = 1; return; }
    de_remove(C, e, sender);
    de_set_owner(C, e, C_INVALID_TILE);
    e->dstate = DS_UNCACHED;
    if (rq_count(H, addr) != 0) {
      c_req* r = rq_front(H, addr);
      dd_front_update_time(r, &t);
      if (r->type == M_EX_REQ) dd_process_ex(C, home, r, 1, &t);
      else if (r->type == M_SH_REQ) { dram_put(C, H, t); dd_process_sh(C, home, r, 1, &t); }
      else { dram_put(C, H, t); dd_process_nullify(C, home, r, &t); }
    } else {
      dram_put(C, H, t);
    }
    break;
  }
  case M_WB_REP: {                               /* processWbRepFromL2Cache (:507-543) */
    c_dentry* e = dc_get(C, H, addr, &t);
    if (!e || e->dstate != DS_MODIFIED || !de_has(e, sender)) { C->err = 1; return; }
    de_set_owner(C, e, C_INVALID_TILE);
    e->dstate = DS_SHARED;
    if (rq_count(H, addr) != 0) {
      c_req* r = rq_front(H, addr);
      dd_front_update_time(r, &t);
      dram_put(C, H, t);
      if (r->type != M_SH_REQ) { C->err = 1; return; }
      dd_process_sh(C, home, r, 1, &t);
    } else {
      C->err = 1;                                /* "Should not reach here" */
    }
    break;
  }
  default: C->err = 1;
  }
}

/* ---- L1 / L2 controllers (l1_cache_cntlr.cc, l2_cache_cntlr.cc) ---------- */

/* L2CacheCntlr::insertCacheLine (l2:74-116): eviction -> L1 invalidate + FLUSH_REP / INV_REP */
static void l2c_insert(oracle_coh* C, uint32_t tile, uint64_t addr, uint32_t cstate, uint64_t t)
{
  c_tile* Tl = &C->t[tile];
  o_line in = { o_tag(&Tl->c.l2, addr), cstate, GG_LOC_L1D };   /* cached_loc = sender = L1-D */
  o_line ev = o_default_line();
  int eviction = 0; uint64_t ev_addr = 0;
  if (o_insert_line(&Tl->c.l2, addr, &in, &eviction, &ev_addr, &ev)) { C->err = 1; return; }
  if (eviction) {
    int e = 0;
    if (ev.loc != GG_LOC_INVALID) l1_invalidate(&Tl->c, ev_addr, &e);
    if (e) C->err = 1;
    uint32_t home = c_home(C, ev_addr);
    if (ev.cstate == CS_M) c_send(C, tile, home, M_FLUSH_REP, tile, ev_addr, t);
    else if (ev.cstate == CS_S) c_send(C, tile, home, M_INV_REP, tile, ev_addr, t);
    else C->err = 1;
  }
}

/* L2CacheCntlr::insertCacheLineInL1 (l2:133-165) via the Mode-P restatement */
static void l2c_insert_in_l1(oracle_coh* C, uint32_t tile, uint64_t addr, uint32_t cstate)
{
  uint32_t res = 0; int e = 0;
  l2_insert_in_l1(&C->t[tile].c, addr, cstate, &res, &e);
  if (e) C->err = 1;
}

/* L1CacheCntlr::accessCache (l1:182-205) */
static void l1c_access(oracle_coh* C, uint32_t tile, uint64_t addr, int is_write)
{
  int e = 0;
  l1_access_cache(&C->t[tile].c, addr, is_write, &e);
  if (e) C->err = 1;
}

static void c_finish_access(oracle_coh* C, uint32_t tile, uint64_t start, uint64_t end, uint32_t level)
{
  c_tile* Tl = &C->t[tile];
  uint64_t lat = end - start;
  if (C->out) C->out[Tl->rec] = (lat << 2) | level;
  Tl->st[GG_CT_ACCESSES]++;
  Tl->st[GG_CT_LATENCY_PS] += lat;
  Tl->st[level == GG_LVL_L1 ? GG_CT_L1_HITS : level == GG_LVL_L2 ? GG_CT_L2_HITS : GG_CT_L2_MISSES]++;
  Tl->clk = end;
  Tl->st[GG_CT_CLOCK_PS] = end;
  Tl->rec++;
}

/* One access of the core: Core::initiateMemoryAccess (core.cc:139-266) ->
 * MemoryManager::__coreInitiateMemoryAccess (memory_manager.cc:78-99) ->
 * L1CacheCntlr::processMemOpFromCore (l1:89-180), first attempt. */
static void c_app_access(oracle_coh* C, uint32_t tile, uint64_t addr, int is_write, uint64_t s)
{
  c_tile* Tl = &C->t[tile];
  uint64_t t = s;                                /* setCurrTime(curr_time) */
  o_line info = o_default_line();
  o_get_line_info(&Tl->c.l1, addr, &info);         /* operationPermissibleinL1Cache (l1:207-243) */
  int hit = is_write ? cs_writable(info.cstate) : cs_readable(info.cstate);
  o_update_miss_counters(&Tl->c.l1, addr, is_write, !hit);
  if (hit) {
    t += C->lat_l1_data;                         /* incrCurrTime(L1, ACCESS_DATA_AND_TAGS) */
    l1c_access(C, tile, addr, is_write);
    c_finish_access(C, tile, s, t, GG_LVL_L1);
    return;
  }
  t += C->lat_l1_tags;                           /* incrCurrTime(L1, ACCESS_TAGS) */
  if (!C->mosi) {                                /* MOSI keeps the line (…mosi/l1_cache_cntlr.cc:127-135) */
    int e = 0;
    l1_invalidate(&Tl->c, addr, &e);             /* l1:137 */
    if (e) C->err = 1;
  }
  /* L2CacheCntlr::processShmemRequestFromL1Cache (l2:180-224) */
  o_line l2i = o_default_line();
  o_get_line_info(&Tl->c.l2, addr, &l2i);
  uint32_t cstate = l2i.cstate;
  int l2hit = is_write ? cs_writable(cstate) : cs_readable(cstate);
  o_update_miss_counters(&Tl->c.l2, addr, is_write, !l2hit);
  if (l2hit) {
    if (o_access_line(&Tl->c.l2, addr, 0)) C->err = 1;   /* readCacheLine */
    l2c_insert_in_l1(C, tile, addr, cstate);
    l2i.loc = GG_LOC_L1D;                        /* setCachedLoc / setForcedCachedLoc(L1_DCACHE) */
    if (o_set_line_info(&Tl->c.l2, addr, &l2i)) C->err = 1;
    t += C->lat_l2_data;                         /* l1:151-153 */
    t += C->lat_l1_data;
    l1c_access(C, tile, addr, is_write);
    c_finish_access(C, tile, s, t, GG_LVL_L2);
    return;
  }
  t += C->lat_l2_tags;                           /* l1:162 */
  /* sendMsg(self, EX_REQ / SH_REQ from L1) -> L2CacheCntlr::handleMsgFromL1Cache (l2:226-258) */
  if (Tl->out_addr != C_INVALID_ADDR) C->err = 1;
  Tl->out_addr = addr; Tl->out_time = t;
  uint32_t home = c_home(C, addr);
  if (C->mosi) {                                 /* …mosi/l2_cache_cntlr.cc:266-285: the request as is */
    c_send(C, tile, home, is_write ? M_EX_REQ : M_SH_REQ, tile, addr, t);
  } else if (is_write) {                         /* processExReqFromL1Cache (l2:260-282) */
    o_line x = o_default_line();
    o_get_line_info(&Tl->c.l2, addr, &x);
    if (x.cstate == CS_S) {
      x.tag = O_INVALID_TAG; x.cstate = CS_I; x.loc = GG_LOC_INVALID;
      if (o_set_line_info(&Tl->c.l2, addr, &x)) C->err = 1;
      c_send(C, tile, home, M_INV_REP, tile, addr, t);
    } else if (x.cstate != CS_I) C->err = 1;
    c_send(C, tile, home, M_EX_REQ, tile, addr, t);
  } else {                                       /* processShReqFromL1Cache (l2:284-292) */
    c_send(C, tile, home, M_SH_REQ, tile, addr, t);
  }
  Tl->blocked = 1;                               /* waitForSimThread */
  Tl->pend_start = s;
}

/* L2CacheCntlr::handleMsgFromDramDirectory (l2:294-347) + the L1's second attempt (l1:106-126) */
static void l2c_handle(oracle_coh* C, uint32_t tile, const gg_cmsg* m)
{
  c_tile* Tl = &C->t[tile];
  uint64_t t = m->arrival_ps;
  uint64_t addr = m->addr;
  uint32_t sender = m->src;
  switch (m->type) {
  case M_EX_REP:
  case M_SH_REP: {
    uint32_t cs = (m->type == M_EX_REP) ? CS_M : CS_S;
    if (!Tl->blocked || Tl->out_addr != addr) { C->err = 1; return; }
    l2c_insert(C, tile, addr, cs, t);            /* insertCacheLineInHierarchy (l2:167-178) */
    l2c_insert_in_l1(C, tile, addr, cs);
    if (Tl->out_time > t) C->err = 1;
    t += C->lat_l2_data;                         /* incrCurrTime(L2, ACCESS_DATA_AND_TAGS) */
    Tl->out_addr = C_INVALID_ADDR;
    /* wakeUpAppThread: the core's second attempt (access_num == 2) */
    const int is_write = (int)(C->meta[Tl->rec] & GG_META_WRITE);
    o_line info = o_default_line();
    o_get_line_info(&Tl->c.l1, addr, &info);
    int hit = is_write ? cs_writable(info.cstate) : cs_readable(info.cstate);
    if (!hit) { C->err = 1; return; }
    t += C->lat_l1_data;
    l1c_access(C, tile, addr, is_write);
    Tl->blocked = 0;
    c_finish_access(C, tile, Tl->pend_start, t, GG_LVL_DIR);
    break;
  }
  case M_INV_REQ: {                              /* processInvReqFromDramDirectory (l2:369-410) */
    o_line l2i = o_default_line();
    o_get_line_info(&Tl->c.l2, addr, &l2i);
    if (l2i.cstate != CS_I) {
      if (l2i.cstate != CS_S) { C->err = 1; return; }
      t += C->lat_l2_tags;
      if (l2i.loc == GG_LOC_L1D) t += C->lat_l1_tags;
      if (l2i.loc != GG_LOC_INVALID) {
        int e = 0;
        l1_invalidate(&Tl->c, addr, &e);
        if (e) C->err = 1;
      }
      l2i.tag = O_INVALID_TAG; l2i.cstate = CS_I; l2i.loc = GG_LOC_INVALID;
      if (o_set_line_info(&Tl->c.l2, addr, &l2i)) C->err = 1;
      c_send(C, tile, sender, M_INV_REP, m->requester, addr, t);
    } else {
      t += C->lat_l2_tags;
    }
    break;
  }
  case M_FLUSH_REQ:                              /* processFlushReqFromDramDirectory (l2:412-455) */
  case M_WB_REQ: {                               /* processWbReqFromDramDirectory (l2:457-502) */
    o_line l2i = o_default_line();
    o_get_line_info(&Tl->c.l2, addr, &l2i);
    if (l2i.cstate != CS_I) {
      if (l2i.cstate != CS_M) { C->err = 1; return; }
      t += C->lat_l2_data;
      if (l2i.loc == GG_LOC_L1D) t += C->lat_l1_tags;
      if (m->type == M_FLUSH_REQ) {
        if (l2i.loc != GG_LOC_INVALID) {
          int e = 0;
          l1_invalidate(&Tl->c, addr, &e);
          if (e) C->err = 1;
        }
        if (o_access_line(&Tl->c.l2, addr, 0)) C->err = 1;        /* readCacheLine */
        l2i.tag = O_INVALID_TAG; l2i.cstate = CS_I; l2i.loc = GG_LOC_INVALID;
        if (o_set_line_info(&Tl->c.l2, addr, &l2i)) C->err = 1;
        c_send(C, tile, sender, M_FLUSH_REP, m->requester, addr, t);
      } else {
        if (l2i.loc != GG_LOC_INVALID) {         /* setCacheLineStateInL1(SHARED) (l1:278-291) */
          o_line l1i = o_default_line();
          o_get_line_info(&Tl->c.l1, addr, &l1i);
          if (l1i.cstate == CS_I) C->err = 1;
          l1i.cstate = CS_S;
          if (o_set_line_info(&Tl->c.l1, addr, &l1i)) C->err = 1;
        }
        if (o_access_line(&Tl->c.l2, addr, 0)) C->err = 1;        /* readCacheLine */
        l2i.cstate = CS_S;
        if (o_set_line_info(&Tl->c.l2, addr, &l2i)) C->err = 1;
        c_send(C, tile, sender, M_WB_REP, m->requester, addr, t);
      }
    } else {
      t += C->lat_l2_tags;
    }
    break;
  }
  default: C->err = 1;
  }
}

/* ==== pr_l1_pr_l2_dram_directory_mosi ====================================
 * The MOSI controllers (…mosi/dram_directory_cntlr.cc, l2_cache_cntlr.cc,
 * l1_cache_cntlr.cc) on the same directory cache, DRAM, clock and network as
 * the MSI restatement above.  Differences that shape results: OWNED lines and
 * entries; UPGRADE_REP for a lone sharer/owner; INV_FLUSH_COMBINED_REQ (one
 * sharer flushes, the others invalidate); SH_REQs served by a sharer's
 * write-back; the directory's cached data list standing in for DRAM; no L1
 * invalidate before a miss goes to the L2; the ShmemReq event/latency counters. */
#define DS_OWNED 3                                /* DirectoryState::OWNED (directory_state.h) */
#define CS_O GG_CSTATE_OWNED
#define NO_TILE ((int32_t)-1)

/* DirectoryEntryFullMap::getOneSharer (directory_entry_full_map.cc:67-74):
 * index = Random<int>::next(#sharers) (misc/random.h:25-31) over drand48_r —
 * X <- (0x5DEECE66D X + 0xB) mod 2^48, result = X / 2^48 (exact in a double),
 * index = (int)(result * n) — into the ascending sharers list. */
static int32_t mo_one_sharer(oracle_coh* C, c_dentry* e)
{
  const uint32_t n = de_num(C, e);
  e->rng = (0x5DEECE66Dull * e->rng + 0xBull) & 0xFFFFFFFFFFFFull;
  const double r = ldexp((double)e->rng, -48);
  uint32_t k = (uint32_t)(int)(r * (double)(int)n);
  for (uint32_t s = 0; s < C->T; ++s)
    if (de_has(e, s) && k-- == 0) return (int32_t)s;
  C->err = 1;                                     /* sharers_list[index] of an empty list */
  return 0;
}

/* DataList (…mosi/dram_directory_cntlr.cc:1196-1241): the line data itself is not modeled */
static int cdl_find(const c_tile* H, uint64_t a)
{
  for (uint32_t i = 0; i < H->ncdl; ++i) if (H->cdl[i] == a) return (int)i;
  return -1;
}
static void cdl_insert(c_tile* H, uint64_t a)
{
  if (cdl_find(H, a) >= 0) return;               /* already present: the same data */
  if (H->ncdl == H->capcdl) { H->capcdl = H->capcdl ? 2 * H->capcdl : 8; H->cdl = (uint64_t*)realloc(H->cdl, 8 * H->capcdl); }
  H->cdl[H->ncdl++] = a;
}
static void cdl_erase(oracle_coh* C, c_tile* H, uint64_t a)
{
  const int i = cdl_find(H, a);
  if (i < 0) { C->err = 1; return; }
  H->cdl[i] = H->cdl[--H->ncdl];
}

static c_req mo_req(uint64_t addr, uint32_t type, uint32_t requester, uint64_t t)   /* ShmemReq(msg, time) (shmem_req.cc:8-22) */
{
  c_req r;
  memset(&r, 0, sizeof(r));
  r.addr = addr; r.type = type; r.requester = requester;
  r.arrival = r.start = r.time = t;
  r.init_ds = DS_UNCACHED; r.sharer = NO_TILE; r.upgrade = 0;
  return r;
}
static void mo_start(c_req* r, uint64_t t)       /* updateProcessingStartTime (shmem_req.cc:26-33) */
{
  if (r->start < t) { r->start = t; r->time = t; }
}
static void mo_finish(c_req* r, uint64_t t)      /* updateProcessingFinishTime (shmem_req.cc:35-40) */
{
  if (r->time < t) r->time = t;
}

/* updateShmemReqEventCounters (:879-965), models enabled */
static void mo_event(oracle_coh* C, c_tile* H, c_req* r, c_dentry* e)
{
  uint64_t* p = H->ps;
  const uint32_t ds = e->dstate, n = de_num(C, e);
  const int shared = ds == DS_OWNED || ds == DS_SHARED;
  if (r->type == M_EX_REQ) {
    p[GG_PS_EXREQ]++;
    if (ds == DS_MODIFIED) p[GG_PS_EXREQ_MODIFIED]++;
    else if (shared) {
      p[GG_PS_EXREQ_SHARED]++;
      if (n == 1 && mo_one_sharer(C, e) == (int32_t)r->requester) { r->upgrade = 1; p[GG_PS_EXREQ_UPGRADE]++; }
      else { p[GG_PS_INV_UNICAST]++; p[GG_PS_INV_SHARERS_UNICAST] += n; }   /* updateInvalidationEventCounters (:967-980) */
    } else p[GG_PS_EXREQ_UNCACHED]++;
  } else if (r->type == M_SH_REQ) {
    p[GG_PS_SHREQ]++;
    p[ds == DS_MODIFIED ? GG_PS_SHREQ_MODIFIED : shared ? GG_PS_SHREQ_SHARED : GG_PS_SHREQ_UNCACHED]++;
  } else {
    p[GG_PS_NULLIFY]++;
    if (ds == DS_MODIFIED) p[GG_PS_NULLIFY_MODIFIED]++;
    else if (shared) { p[GG_PS_NULLIFY_SHARED]++; p[GG_PS_INV_UNICAST]++; p[GG_PS_INV_SHARERS_UNICAST] += n; }
    else p[GG_PS_NULLIFY_UNCACHED]++;
  }
}
/* updateShmemReqLatencyCounters (:982-1014) of a completed request */
static void mo_latency(c_tile* H, const c_req* r)
{
  uint64_t* p = H->ps;
  const uint64_t ser = r->start - r->arrival, proc = r->time - r->start;
  const int inv0 = r->init_ds == DS_OWNED || r->init_ds == DS_SHARED;
  if (r->type == M_EX_REQ) {
    p[GG_PS_EXREQ_SERIALIZATION_PS] += ser; p[GG_PS_EXREQ_PROCESSING_PS] += proc;
    if (inv0 && !r->upgrade) p[GG_PS_INV_PROCESSING_UNICAST_PS] += proc;
  } else if (r->type == M_SH_REQ) {
    p[GG_PS_SHREQ_SERIALIZATION_PS] += ser; p[GG_PS_SHREQ_PROCESSING_PS] += proc;
  } else {
    p[GG_PS_NULLIFY_SERIALIZATION_PS] += ser; p[GG_PS_NULLIFY_PROCESSING_PS] += proc;
    if (inv0) p[GG_PS_INV_PROCESSING_UNICAST_PS] += proc;
  }
}

static void mo_process_ex(oracle_coh* C, uint32_t home, c_req* req, c_dentry* e, int first, uint64_t* t);
static void mo_process_sh(oracle_coh* C, uint32_t home, c_req* req, c_dentry* e, int first, uint64_t* t);
static void mo_process_nullify(oracle_coh* C, uint32_t home, c_req* req, c_dentry* e, int first, uint64_t* t);

/* sendShmemMsg (:535-561): full map never reports all tiles sharers -> one message per sharer, ascending */
static void mo_send_sharers(oracle_coh* C, uint32_t home, uint32_t type, uint64_t addr, uint32_t requester,
                            int32_t single, const c_dentry* e, uint64_t t)
{
  for (uint32_t s = 0; s < C->T; ++s)
    if (de_has(e, s)) c_send_rx(C, home, s, type, requester, addr, t, (uint32_t)single);
}

/* retrieveDataAndSendToL2Cache (:563-595) */
static void mo_retrieve_and_send(oracle_coh* C, uint32_t home, uint32_t type, uint32_t receiver, uint64_t addr, uint64_t* t)
{
  c_tile* H = &C->t[home];
  if (cdl_find(H, addr) >= 0) {
    c_send(C, home, receiver, type, receiver, addr, *t);
    cdl_erase(C, H, addr);
  } else {
    dram_get(C, H, t);
    c_send(C, home, receiver, type, receiver, addr, *t);
  }
}

/* processNextReqFromL2Cache (:117-163) */
static void mo_next(oracle_coh* C, uint32_t home, uint64_t addr, uint64_t* t)
{
  c_tile* H = &C->t[home];
  if (rq_count(H, addr) < 1) { C->err = 1; return; }
  c_req* done = rq_front(H, addr);
  mo_finish(done, *t);
  mo_latency(H, done);
  rq_dequeue(H, addr);
  if (cdl_find(H, addr) >= 0) C->err = 1;        /* assert(_cached_data_list.lookup(address) == NULL) */
  c_req* r = rq_front(H, addr);
  if (r) {
    mo_start(r, *t);
    if (*t < r->time) *t = r->time;              /* updateCurrTime(getTime()) */
    if (r->type == M_EX_REQ) mo_process_ex(C, home, r, NULL, 1, t);
    else if (r->type == M_SH_REQ) mo_process_sh(C, home, r, NULL, 1, t);
    else C->err = 1;
  }
}

/* processDirectoryEntryAllocationReq (:165-209) */
static c_dentry* mo_allocate(oracle_coh* C, uint32_t home, const c_req* req, uint64_t* t)
{
  c_tile* H = &C->t[home];
  const uint64_t addr = req->addr, msg_time = *t;
  const uint32_t requester = req->requester;
  if (dc_get(C, H, addr, t) != NULL) C->err = 1;  /* getReplacementCandidates' assert (directory_cache.cc:161) */
  const uint32_t set = dc_set(C, addr);
  c_dentry* cand = NULL;
  for (uint32_t i = 0; i < C->dir_assoc; ++i) {
    c_dentry* it = dc_slot(C, H, (size_t)set * C->dir_assoc + i);
    if ((cand == NULL || de_num(C, cand) > de_num(C, it)) && rq_count(H, it->addr) == 0) cand = it;
  }
  if (!cand) { C->err = 1; return NULL; }
  const uint64_t replaced_addr = cand->addr;
  c_dentry* e = dc_replace(C, H, replaced_addr, addr, t);   /* the new entry: a fresh Random */
  c_req* nr = rq_enqueue(H, mo_req(replaced_addr, M_NULLIFY_REQ, requester, msg_time));
  if (rq_count(H, replaced_addr) != 1) C->err = 1;
  mo_process_nullify(C, home, nr, NULL, 1, t);
  return e;
}

/* processNullifyReq (:211-297) */
static void mo_process_nullify(oracle_coh* C, uint32_t home, c_req* req, c_dentry* e, int first, uint64_t* t)
{
  c_tile* H = &C->t[home];
  const uint64_t addr = req->addr;
  const uint32_t requester = req->requester;
  if (!e) e = dc_get(C, H, addr, t);
  if (!e) { C->err = 1; return; }
  if (first) { req->init_ds = e->dstate; mo_event(C, H, req, e); }
  switch (e->dstate) {
  case DS_MODIFIED:
    c_send(C, home, (uint32_t)e->owner, M_FLUSH_REQ, requester, addr, *t);
    break;
  case DS_OWNED:
    if (e->owner == C_INVALID_TILE) C->err = 1;
    mo_send_sharers(C, home, GG_MSG_INV_FLUSH_COMBINED_REQ, addr, requester, e->owner, e, *t);
    break;
  case DS_SHARED:
    if (e->owner != C_INVALID_TILE) C->err = 1;
    mo_send_sharers(C, home, M_INV_REQ, addr, requester, NO_TILE, e, *t);
    break;
  case DS_UNCACHED:
    if (cdl_find(H, addr) >= 0) { dram_put(C, H, *t); cdl_erase(C, H, addr); }   /* sendDataToDram */
    dc_invalidate(C, H, addr);
    mo_next(C, home, addr, t);
    break;
  default: C->err = 1;
  }
}

/* processExReqFromL2Cache (:299-421) */
static void mo_process_ex(oracle_coh* C, uint32_t home, c_req* req, c_dentry* e, int first, uint64_t* t)
{
  c_tile* H = &C->t[home];
  const uint64_t addr = req->addr;
  const uint32_t requester = req->requester;
  if (!e) e = dc_get(C, H, addr, t);
  if (!e) { e = mo_allocate(C, home, req, t); if (!e) return; }
  if (first) { req->init_ds = e->dstate; mo_event(C, H, req, e); }
  const uint32_t n = de_num(C, e);
  switch (e->dstate) {
  case DS_MODIFIED:
    c_send(C, home, (uint32_t)e->owner, M_FLUSH_REQ, requester, addr, *t);
    break;
  case DS_OWNED:
    if (e->owner == (int32_t)requester && n == 1) {
      e->dstate = DS_MODIFIED;
      c_send(C, home, requester, GG_MSG_UPGRADE_REP, requester, addr, *t);
      mo_next(C, home, addr, t);
    } else {
      mo_send_sharers(C, home, GG_MSG_INV_FLUSH_COMBINED_REQ, addr, requester, e->owner, e, *t);
    }
    break;
  case DS_SHARED:
    if (n == 0) C->err = 1;
    if (de_has(e, requester) && n == 1) {
      de_set_owner(C, e, (int32_t)requester);
      e->dstate = DS_MODIFIED;
      c_send(C, home, requester, GG_MSG_UPGRADE_REP, requester, addr, *t);
      mo_next(C, home, addr, t);
    } else {
      const int32_t one = mo_one_sharer(C, e);
      mo_send_sharers(C, home, GG_MSG_INV_FLUSH_COMBINED_REQ, addr, requester, one, e, *t);
    }
    break;
  case DS_UNCACHED:
    if (n != 0) C->err = 1;
    de_add(C, e, requester);
    de_set_owner(C, e, (int32_t)requester);
    e->dstate = DS_MODIFIED;
    mo_retrieve_and_send(C, home, M_EX_REP, requester, addr, t);
    mo_next(C, home, addr, t);
    break;
  default: C->err = 1;
  }
}

/* processShReqFromL2Cache (:423-533) */
static void mo_process_sh(oracle_coh* C, uint32_t home, c_req* req, c_dentry* e, int first, uint64_t* t)
{
  c_tile* H = &C->t[home];
  const uint64_t addr = req->addr;
  const uint32_t requester = req->requester;
  if (!e) e = dc_get(C, H, addr, t);
  if (!e) { e = mo_allocate(C, home, req, t); if (!e) return; }
  if (first) { req->init_ds = e->dstate; mo_event(C, H, req, e); }
  switch (e->dstate) {
  case DS_MODIFIED:
    c_send(C, home, (uint32_t)e->owner, M_WB_REQ, requester, addr, *t);
    req->sharer = e->owner;
    break;
  case DS_OWNED:
  case DS_SHARED: {
    if (de_num(C, e) == 0) C->err = 1;
    const int32_t sharer = mo_one_sharer(C, e);   /* the sharer can be the owner */
    de_add(C, e, requester);                      /* full map: always added */
    if (cdl_find(H, addr) < 0 && sharer != NO_TILE) {
      de_remove(C, e, requester);                 /* not complete yet */
      c_send(C, home, (uint32_t)sharer, M_WB_REQ, requester, addr, *t);
      req->sharer = sharer;
    } else {
      mo_retrieve_and_send(C, home, M_SH_REP, requester, addr, t);
      mo_next(C, home, addr, t);
    }
    break;
  }
  case DS_UNCACHED:
    de_add(C, e, requester);
    e->dstate = DS_SHARED;
    mo_retrieve_and_send(C, home, M_SH_REP, requester, addr, t);
    mo_next(C, home, addr, t);
    break;
  default: C->err = 1;
  }
}

/* restartShmemReq (:797-833) */
static void mo_restart(oracle_coh* C, uint32_t home, uint32_t sender, c_req* req, c_dentry* e, uint64_t* t)
{
  mo_finish(req, *t);
  if (*t < req->time) *t = req->time;
  const uint32_t ds = e->dstate;
  if (req->type == M_EX_REQ) {
    if (ds == DS_UNCACHED) mo_process_ex(C, home, req, e, 0, t);
  } else if (req->type == M_SH_REQ) {
    if (req->sharer == NO_TILE) C->err = 1;
    if ((int32_t)sender == req->sharer) { req->sharer = NO_TILE; mo_process_sh(C, home, req, e, 0, t); }
  } else {
    if (ds == DS_UNCACHED) mo_process_nullify(C, home, req, e, 0, t);
  }
}

/* handleMsgFromL2Cache (:49-115) and the replies (:597-795) */
static void mo_dd_handle(oracle_coh* C, uint32_t home, const gg_cmsg* m)
{
  c_tile* H = &C->t[home];
  uint64_t t = m->arrival_ps;
  const uint64_t addr = m->addr;
  const uint32_t sender = m->src;
  switch (m->type) {
  case M_EX_REQ:
  case M_SH_REQ: {
    c_req* r = rq_enqueue(H, mo_req(addr, m->type, m->requester, t));
    if (rq_count(H, addr) == 1) {
      mo_start(r, t);
      if (cdl_find(H, addr) >= 0) C->err = 1;
      if (m->type == M_EX_REQ) mo_process_ex(C, home, r, NULL, 1, &t);
      else mo_process_sh(C, home, r, NULL, 1, &t);
    }
    break;
  }
  case M_INV_REP: {                              /* processInvRepFromL2Cache (:597-643) */
    c_dentry* e = dc_get(C, H, addr, &t);
    if (!e) { C->err = 1; return; }
    if (e->dstate == DS_OWNED) {
      if ((int32_t)sender == e->owner || de_num(C, e) == 0) C->err = 1;
      de_remove(C, e, sender);
      if (de_num(C, e) == 0) C->err = 1;
    } else if (e->dstate == DS_SHARED) {
      if (e->owner != C_INVALID_TILE || de_num(C, e) == 0) C->err = 1;
      de_remove(C, e, sender);
      if (de_num(C, e) == 0) e->dstate = DS_UNCACHED;
    } else { C->err = 1; return; }
    if (rq_count(H, addr) > 0) mo_restart(C, home, sender, rq_front(H, addr), e, &t);
    break;
  }
  case M_FLUSH_REP: {                            /* processFlushRepFromL2Cache (:645-734) */
    c_dentry* e = dc_get(C, H, addr, &t);
    if (!e) { C->err = 1; return; }
    const uint32_t ds0 = e->dstate;
    if (ds0 == DS_MODIFIED) {
      if ((int32_t)sender != e->owner) C->err = 1;
      de_remove(C, e, sender);
      de_set_owner(C, e, C_INVALID_TILE);
      e->dstate = DS_UNCACHED;
    } else if (ds0 == DS_OWNED) {
      if (e->owner == C_INVALID_TILE || de_num(C, e) == 0) C->err = 1;
      de_remove(C, e, sender);
      if ((int32_t)sender == e->owner) {
        de_set_owner(C, e, C_INVALID_TILE);
        e->dstate = de_num(C, e) > 0 ? DS_SHARED : DS_UNCACHED;
      }
    } else if (ds0 == DS_SHARED) {
      if (e->owner != C_INVALID_TILE || de_num(C, e) == 0) C->err = 1;
      de_remove(C, e, sender);
      if (de_num(C, e) == 0) e->dstate = DS_UNCACHED;
    } else { C->err = 1; return; }
    if (rq_count(H, addr) > 0) {
      cdl_insert(H, addr);
      c_req* r = rq_front(H, addr);
      if (r->type == M_SH_REQ && (ds0 == DS_MODIFIED || ds0 == DS_OWNED) &&
          (e->dstate == DS_SHARED || e->dstate == DS_UNCACHED))
        dram_put(C, H, t);
      mo_restart(C, home, sender, r, e, &t);
    } else {
      dram_put(C, H, t);                         /* just an eviction */
    }
    break;
  }
  case M_WB_REP: {                               /* processWbRepFromL2Cache (:736-795) */
    c_dentry* e = dc_get(C, H, addr, &t);
    if (!e) { C->err = 1; return; }
    if (e->dstate == DS_MODIFIED) {
      if ((int32_t)sender != e->owner || rq_count(H, addr) == 0) C->err = 1;
      e->dstate = DS_OWNED;
    } else if (e->dstate == DS_OWNED) {
      if (!de_has(e, sender)) C->err = 1;
    } else if (e->dstate == DS_SHARED) {
      if (e->owner != C_INVALID_TILE || !de_has(e, sender)) C->err = 1;
    } else { C->err = 1; return; }
    if (rq_count(H, addr) > 0) {
      cdl_insert(H, addr);
      mo_restart(C, home, sender, rq_front(H, addr), e, &t);
    } else {
      C->err = 1;                                /* "WB_REP, NO requester" */
    }
    break;
  }
  default: C->err = 1;
  }
}

/* L2CacheCntlr::insertCacheLine (…mosi/l2_cache_cntlr.cc:95-149) + updateEvictionCounters (:605-636) */
static void mo_l2_insert(oracle_coh* C, uint32_t tile, uint64_t addr, uint32_t cstate, uint64_t t)
{
  c_tile* Tl = &C->t[tile];
  o_line in = { o_tag(&Tl->c.l2, addr), cstate, GG_LOC_L1D };
  o_line ev = o_default_line();
  int eviction = 0; uint64_t ev_addr = 0;
  if (o_insert_line(&Tl->c.l2, addr, &in, &eviction, &ev_addr, &ev)) { C->err = 1; return; }
  if (!eviction) return;
  const int dirty = ev.cstate == CS_M || ev.cstate == CS_O;
  if (!dirty && ev.cstate != CS_S) { C->err = 1; return; }
  Tl->ps[GG_PS_L2_EVICTIONS]++;
  if (cstate == CS_M) Tl->ps[dirty ? GG_PS_L2_DIRTY_EVICTIONS_EXREQ : GG_PS_L2_CLEAN_EVICTIONS_EXREQ]++;
  else Tl->ps[dirty ? GG_PS_L2_DIRTY_EVICTIONS_SHREQ : GG_PS_L2_CLEAN_EVICTIONS_SHREQ]++;
  if (ev.loc != GG_LOC_INVALID) {
    int e = 0;
    l1_invalidate(&Tl->c, ev_addr, &e);
    if (e) C->err = 1;
  }
  c_send(C, tile, c_home(C, ev_addr), dirty ? M_FLUSH_REP : M_INV_REP, tile, ev_addr, t);
}

/* L1CacheCntlr::setCacheLineState (…mosi/l1_cache_cntlr.cc:260-273) */
static void mo_l1_set_state(oracle_coh* C, uint32_t tile, uint64_t addr, uint32_t cstate)
{
  c_tile* Tl = &C->t[tile];
  o_line l1i = o_default_line();
  o_get_line_info(&Tl->c.l1, addr, &l1i);
  if (l1i.cstate == CS_I) C->err = 1;
  l1i.cstate = cstate;
  if (o_set_line_info(&Tl->c.l1, addr, &l1i)) C->err = 1;
}

/* invalidateCacheLine (L2, :76-81) */
static void mo_l2_invalidate(oracle_coh* C, uint32_t tile, uint64_t addr, o_line* l2i)
{
  l2i->tag = O_INVALID_TAG; l2i->cstate = CS_I; l2i->loc = GG_LOC_INVALID;
  if (o_set_line_info(&C->t[tile].c.l2, addr, l2i)) C->err = 1;
}

/* L2CacheCntlr::handleMsgFromDramDirectory (…mosi/l2_cache_cntlr.cc:287-348) */
static void mo_l2_handle(oracle_coh* C, uint32_t tile, const gg_cmsg* m)
{
  c_tile* Tl = &C->t[tile];
  uint64_t t = m->arrival_ps;
  const uint64_t addr = m->addr;
  const uint32_t sender = m->src;
  uint32_t type = m->type;
  if (type == GG_MSG_INV_FLUSH_COMBINED_REQ)      /* processInvFlushCombinedReqFromDramDirectory (:581-594) */
    type = m->single_rx == tile ? M_FLUSH_REQ : M_INV_REQ;
  switch (type) {
  case M_EX_REP:
  case M_SH_REP:
  case GG_MSG_UPGRADE_REP: {
    if (!Tl->blocked || Tl->out_addr != addr) { C->err = 1; return; }
    if (type != GG_MSG_UPGRADE_REP) {            /* insertCacheLineInHierarchy (:210-224) */
      const uint32_t cs = type == M_EX_REP ? CS_M : CS_S;
      mo_l2_insert(C, tile, addr, cs, t);
      l2c_insert_in_l1(C, tile, addr, cs);
    } else {                                     /* processUpgradeRepFromDramDirectory (:370-412) */
      o_line l2i = o_default_line();
      o_get_line_info(&Tl->c.l2, addr, &l2i);
      if (l2i.cstate != CS_S && l2i.cstate != CS_O) C->err = 1;
      l2i.cstate = CS_M;
      if (l2i.loc == GG_LOC_INVALID) {
        if (o_access_line(&Tl->c.l2, addr, 0)) C->err = 1;   /* readCacheLine */
        l2c_insert_in_l1(C, tile, addr, CS_M);
        l2i.loc = GG_LOC_L1D;
      } else {
        mo_l1_set_state(C, tile, addr, CS_M);
      }
      if (o_set_line_info(&Tl->c.l2, addr, &l2i)) C->err = 1;
    }
    if (Tl->out_time > t) C->err = 1;
    t += C->lat_l2_data;                         /* incrCurrTime(L2, ACCESS_DATA_AND_TAGS) */
    Tl->out_addr = C_INVALID_ADDR;
    /* wakeUpAppThread: the core's second attempt (l1:105-126, access_num == 2) */
    const int is_write = (int)(C->meta[Tl->rec] & GG_META_WRITE);
    o_line info = o_default_line();
    o_get_line_info(&Tl->c.l1, addr, &info);
    if (!(is_write ? cs_writable(info.cstate) : cs_readable(info.cstate))) { C->err = 1; return; }
    t += C->lat_l1_data;
    l1c_access(C, tile, addr, is_write);
    Tl->blocked = 0;
    c_finish_access(C, tile, Tl->pend_start, t, GG_LVL_DIR);
    break;
  }
  case M_INV_REQ: {                              /* processInvReqFromDramDirectory (:414-468) */
    o_line l2i = o_default_line();
    o_get_line_info(&Tl->c.l2, addr, &l2i);
    t += C->lat_l2_tags;
    if (l2i.cstate == CS_I) break;               /* full map: no reply expected */
    if (l2i.cstate != CS_S) { C->err = 1; return; }
    if (l2i.loc == GG_LOC_L1D) t += C->lat_l1_tags;
    Tl->ps[GG_PS_L2_INVALIDATIONS]++;
    if (l2i.loc != GG_LOC_INVALID) { int e = 0; l1_invalidate(&Tl->c, addr, &e); if (e) C->err = 1; }
    mo_l2_invalidate(C, tile, addr, &l2i);
    c_send(C, tile, sender, M_INV_REP, m->requester, addr, t);
    break;
  }
  case M_FLUSH_REQ: {                            /* processFlushReqFromDramDirectory (:470-527) */
    o_line l2i = o_default_line();
    o_get_line_info(&Tl->c.l2, addr, &l2i);
    if (l2i.cstate == CS_I) { t += C->lat_l2_tags; break; }
    t += C->lat_l2_data;
    if (l2i.loc == GG_LOC_L1D) t += C->lat_l1_tags;
    Tl->ps[GG_PS_L2_INVALIDATIONS]++;            /* (MODIFIED, OWNED, SHARED) -> INVALID */
    if (l2i.loc != GG_LOC_INVALID) { int e = 0; l1_invalidate(&Tl->c, addr, &e); if (e) C->err = 1; }
    if (o_access_line(&Tl->c.l2, addr, 0)) C->err = 1;      /* readCacheLine */
    mo_l2_invalidate(C, tile, addr, &l2i);
    c_send(C, tile, sender, M_FLUSH_REP, m->requester, addr, t);
    break;
  }
  case M_WB_REQ: {                               /* processWbReqFromDramDirectory (:529-579) */
    o_line l2i = o_default_line();
    o_get_line_info(&Tl->c.l2, addr, &l2i);
    if (l2i.cstate == CS_I) { t += C->lat_l2_tags; break; }
    t += C->lat_l2_data;
    if (l2i.loc == GG_LOC_L1D) t += C->lat_l1_tags;
    const uint32_t ns = l2i.cstate == CS_M ? CS_O : l2i.cstate;  /* M -> O, O -> O, S -> S */
    if (l2i.loc != GG_LOC_INVALID) mo_l1_set_state(C, tile, addr, ns);
    if (o_access_line(&Tl->c.l2, addr, 0)) C->err = 1;      /* readCacheLine */
    l2i.cstate = ns;
    if (o_set_line_info(&Tl->c.l2, addr, &l2i)) C->err = 1;
    c_send(C, tile, sender, M_WB_REP, m->requester, addr, t);
    break;
  }
  default: C->err = 1;
  }
}

/* ==== pr_l1_sh_l2_msi ======================================================
 * Private L1-Ds; the L2 is one slice per tile (home = line % tiles,
 * …sh_l2_msi/memory_manager.cc:128-132), each L2 line carrying its full-map
 * directory entry; a miss is an EX_REQ / SH_REQ from the L1 straight to the
 * home slice, which fetches from / stores to the DRAM controller of the
 * line's DRAM home (the same tile) by DRAM_FETCH / DRAM_STORE messages.
 * L1CacheCntlr (…sh_l2_msi/l1_cache_cntlr.cc), L2CacheCntlr (l2_cache_cntlr.cc),
 * DramCntlr (dram_cntlr.cc), L2CacheReplacementPolicy and L2CacheHashFn. */
enum { CS_DATA_INVALID = 5, CS_CLEAN = 6, CS_DIRTY = 7 };   /* CacheState::Type (cache_state.h:11-22) */
#define SH_NULL_DATA 0                                      /* a message without a data buffer */

/* L2CacheHashFn::compute (l2_cache_hash_fn.cc:18-34): XOR of log2(sets)-bit fields above the line offset */
static uint32_t sh_set(const oracle_coh* C, uint64_t addr)
{
  if (C->log_l2_sets == 0) return 0;
  uint64_t set = 0;
  const uint64_t mask = (1ull << C->log_l2_sets) - 1;
  for (uint32_t i = C->log_line; i + C->log_l2_sets <= 64; i += C->log_l2_sets) set ^= (addr >> i) & mask;
  return (uint32_t)set;
}
/* the slice's Cache operations (cache.cc) with the protocol's hash: line index or -1 */
static long sh_find(const oracle_coh* C, const c_tile* H, uint64_t addr)
{
  const o_cache* c = &H->c.l2;
  const uint32_t s = sh_set(C, addr);
  const int w = o_find(c, s, addr >> c->log_line);
  return w < 0 ? -1 : (long)((size_t)s * c->ways + (uint32_t)w);
}
/* Cache::getCacheLineInfo: the caller's default when absent */
static void sh_cache_get(oracle_coh* C, c_tile* H, uint64_t addr, o_line* info, c_dentry** de)
{
  const long i = sh_find(C, H, addr);
  if (i >= 0) { *info = H->c.l2.lines[i]; *de = H->sde[i]; }
  H->c.l2.c[GG_CC_TAG_READS]++;
}
static void sh_cache_set(oracle_coh* C, c_tile* H, uint64_t addr, const o_line* info, c_dentry* de)
{
  const long i = sh_find(C, H, addr);
  if (i < 0) { C->err = 1; return; }
  H->c.l2.lines[i] = *info; H->sde[i] = de;
  H->c.l2.c[GG_CC_TAG_WRITES]++;
}
/* Cache::accessCacheLine: read / write of the line's data (the L2 policy's update is a no-op) */
static void sh_cache_access(oracle_coh* C, c_tile* H, uint64_t addr, int store)
{
  if (sh_find(C, H, addr) < 0) { C->err = 1; return; }
  H->c.l2.c[store ? GG_CC_DATA_WRITES : GG_CC_DATA_READS]++;
}
/* L2CacheReplacementPolicy::getReplacementWay (l2_cache_replacement_policy.cc:20-67):
 * the first INVALID way, else the fewest sharers among lines no request waits on */
static int sh_victim(oracle_coh* C, c_tile* H, uint32_t set)
{
  const o_cache* c = &H->c.l2;
  int way = -1;
  int64_t mn = (int64_t)C->T + 2 + 1;                         /* Config::getTotalTiles() + 1 */
  for (uint32_t i = 0; i < c->ways; ++i) {
    const size_t k = (size_t)set * c->ways + i;
    if (c->lines[k].cstate == CS_I) return (int)i;
    const uint64_t a = c->lines[k].tag << c->log_line;
    const int64_t n = (int64_t)de_num(C, H->sde[k]);
    if (n < mn && rq_count(H, a) == 0) { mn = n; way = (int)i; }
  }
  return way;                                                 /* LOG_ASSERT_ERROR "Could not find a replacement candidate" */
}
/* Cache::insertCacheLine + CacheSet::insert (cache_set.cc:72-103) on the slice */
static void sh_cache_insert(oracle_coh* C, c_tile* H, uint64_t addr, const o_line* in, c_dentry* de, int* ev,
                            uint64_t* ev_addr, o_line* ev_line, c_dentry** ev_de)
{
  o_cache* c = &H->c.l2;
  const uint32_t s = sh_set(C, addr);
  const int w = sh_victim(C, H, s);
  if (w < 0) { C->err = 1; *ev = 0; return; }                /* assert(index < _associativity) */
  const size_t k = (size_t)s * c->ways + (uint32_t)w;
  *ev = c->lines[k].tag != O_INVALID_TAG;
  if (*ev) { *ev_line = c->lines[k]; *ev_de = H->sde[k]; *ev_addr = ev_line->tag << c->log_line; }
  c->lines[k] = *in; H->sde[k] = de;
  if (*ev) {
    c->c[GG_CC_TAG_READS]++; c->c[GG_CC_DATA_READS]++; c->c[GG_CC_EVICTIONS]++;
    if (ev_line->cstate == CS_M || ev_line->cstate == GG_CSTATE_OWNED || ev_line->cstate == CS_DIRTY)
      c->c[GG_CC_DIRTY_EVICTIONS]++;                          /* CacheState::dirty() */
  } else {
    c->c[GG_CC_TAG_READS]++;
  }
  c->c[GG_CC_TAG_WRITES]++; c->c[GG_CC_DATA_WRITES]++;
}
static long sh_ev_find(const c_tile* H, uint64_t addr)
{
  for (uint32_t i = 0; i < H->nev; ++i) if (H->eva[i] == addr) return (long)i;
  return -1;
}

static void sh_process_ex(oracle_coh* C, uint32_t home, c_req* req, int data, int first, uint64_t* t);
static void sh_process_sh(oracle_coh* C, uint32_t home, c_req* req, int data, int first, uint64_t* t);
static void sh_process_nullify(oracle_coh* C, uint32_t home, c_req* req, int data, uint64_t* t);

/* L2CacheCntlr::allocateCacheLine (l2_cache_cntlr.cc:130-189) */
static void sh_allocate(oracle_coh* C, uint32_t home, uint64_t addr, o_line* info, c_dentry** de, uint64_t* t)
{
  c_tile* H = &C->t[home];
  c_dentry* ne = de_new(C);
  o_line in = { addr >> H->c.l2.log_line, CS_DATA_INVALID, GG_LOC_INVALID };
  *info = in; *de = ne;
  int ev = 0; uint64_t ev_addr = 0; o_line evl = o_default_line(); c_dentry* evd = NULL;
  sh_cache_insert(C, H, addr, &in, ne, &ev, &ev_addr, &evl, &evd);
  if (!ev) return;
  if (rq_count(H, ev_addr) || (evl.cstate != CS_CLEAN && evl.cstate != CS_DIRTY) || !evd) C->err = 1;
  /* a NULLIFY_REQ for the evicted line, queued and processed now (:162-182) */
  c_req r; memset(&r, 0, sizeof(r));
  r.addr = ev_addr; r.time = *t; r.type = M_NULLIFY_REQ; r.requester = home;
  c_req* nq = rq_enqueue(H, r);
  if (H->nev == H->capev) {
    H->capev = H->capev ? 2 * H->capev : 8;
    H->eva = (uint64_t*)realloc(H->eva, sizeof(uint64_t) * H->capev);
    H->evl = (o_line*)realloc(H->evl, sizeof(o_line) * H->capev);
    H->evd = (c_dentry**)realloc(H->evd, sizeof(c_dentry*) * H->capev);
  }
  H->eva[H->nev] = ev_addr; H->evl[H->nev] = evl; H->evd[H->nev] = evd; H->nev++;
  sh_process_nullify(C, home, nq, 1, t);                       /* the writeback buffer of the eviction */
}

/* L2CacheCntlr::getCacheLineInfo (l2_cache_cntlr.cc:65-100) */
static void sh_get_info(oracle_coh* C, uint32_t home, uint64_t addr, uint32_t type, int update_miss, o_line* info,
                        c_dentry** de, uint64_t* t)
{
  c_tile* H = &C->t[home];
  const long e = sh_ev_find(H, addr);
  *info = o_default_line(); *de = NULL;
  if (e < 0) {
    if (type == M_NULLIFY_REQ) C->err = 1;
    sh_cache_get(C, H, addr, info, de);
    if (update_miss) o_update_miss_counters(&H->c.l2, addr, type == M_EX_REQ, info->cstate == CS_I);
    if (info->cstate == CS_I) {
      if (type == M_EX_REQ || type == M_SH_REQ) sh_allocate(C, home, addr, info, de, t);
      else C->err = 1;                                        /* LOG_PRINT_ERROR */
    }
  } else {
    if (update_miss) C->err = 1;
    *info = H->evl[e]; *de = H->evd[e];
  }
}
/* L2CacheCntlr::setCacheLineInfo (:102-116) */
static void sh_set_info(oracle_coh* C, uint32_t home, uint64_t addr, const o_line* info, c_dentry* de)
{
  c_tile* H = &C->t[home];
  const long e = sh_ev_find(H, addr);
  if (e < 0) sh_cache_set(C, H, addr, info, de);
  else { H->evl[e] = *info; H->evd[e] = de; }
}

/* readCacheLineAndSendToL1Cache (:878-905): the L2's copy unless a reply brought the data */
static void sh_read_and_send(oracle_coh* C, uint32_t home, uint32_t type, uint64_t addr, int data, uint32_t requester, uint64_t t)
{
  if (!data) sh_cache_access(C, &C->t[home], addr, 0);
  c_send(C, home, requester, type, requester, addr, t);
}

/* processNextReqFromL1Cache (:305-336) */
static void sh_next(oracle_coh* C, uint32_t home, uint64_t addr, uint64_t* t)
{
  c_tile* H = &C->t[home];
  *t += lat_to_ps(1, C->cfg.frequency_ghz);                   /* Latency(1, L2 frequency) */
  if (rq_count(H, addr) < 1) { C->err = 1; return; }
  rq_dequeue(H, addr);
  c_req* f = rq_front(H, addr);
  if (!f) return;
  if (f->time < *t) f->time = *t;                             /* updateTime */
  if (*t < f->time) *t = f->time;                             /* updateCurrTime */
  if (f->type == M_EX_REQ) sh_process_ex(C, home, f, SH_NULL_DATA, 1, t);   /* processShmemReq (:338-356) */
  else if (f->type == M_SH_REQ) sh_process_sh(C, home, f, SH_NULL_DATA, 1, t);
  else C->err = 1;
}

/* processNullifyReq (:358-440) */
static void sh_process_nullify(oracle_coh* C, uint32_t home, c_req* req, int data, uint64_t* t)
{
  const uint64_t addr = req->addr;
  o_line info; c_dentry* e;
  sh_get_info(C, home, addr, M_NULLIFY_REQ, 0, &info, &e, t);
  if (info.cstate == CS_I || !e) { C->err = 1; return; }
  int completed = 0;
  const uint32_t dram = c_home(C, addr);
  if (e->dstate == DS_MODIFIED) {                             /* (MESI: EXCLUSIVE, the owner invalidated) */
    c_send(C, home, (uint32_t)e->owner, C->mesi ? M_INV_REQ : M_FLUSH_REQ, req->requester, addr, *t);
  } else if (e->dstate == DS_SHARED) {
    for (uint32_t w = 0; w < C->sharer_words; ++w)             /* getSharersList, ascending */
      for (uint64_t b = e->sharers[w]; b; b &= b - 1)
        c_send(C, home, w * 64 + (uint32_t)__builtin_ctzll(b), M_INV_REQ, req->requester, addr, *t);
    if (info.cstate == CS_DIRTY && data) c_send(C, home, dram, GG_MSG_DRAM_STORE_REQ, req->requester, addr, *t);
  } else {
    if (info.cstate == CS_DIRTY && data) c_send(C, home, dram, GG_MSG_DRAM_STORE_REQ, req->requester, addr, *t);
    completed = 1;
  }
  if (completed) {
    c_tile* H = &C->t[home];
    sh_set_info(C, home, addr, &info, e);
    const long k = sh_ev_find(H, addr);                      /* delete the entry, erase the evicted line */
    de_free(e);
    if (k >= 0) {
      memmove(&H->eva[k], &H->eva[k + 1], sizeof(uint64_t) * (H->nev - k - 1));
      memmove(&H->evl[k], &H->evl[k + 1], sizeof(o_line) * (H->nev - k - 1));
      memmove(&H->evd[k], &H->evd[k + 1], sizeof(c_dentry*) * (H->nev - k - 1));
      H->nev--;
    } else C->err = 1;
    sh_next(C, home, addr, t);
  }
}

/* processExReqFromL1Cache (:442-562) */
static void sh_process_ex(oracle_coh* C, uint32_t home, c_req* req, int data, int first, uint64_t* t)
{
  const uint64_t addr = req->addr;
  const uint32_t rq = req->requester;
  o_line info; c_dentry* e;
  sh_get_info(C, home, addr, M_EX_REQ, first, &info, &e, t);
  if (info.cstate == CS_I || !e) { C->err = 1; return; }
  int completed = 0;
  if (info.cstate != CS_DATA_INVALID) {
    if (e->dstate == DS_MODIFIED) {
      c_send(C, home, (uint32_t)e->owner, C->mesi ? M_INV_REQ : M_FLUSH_REQ, rq, addr, *t);
    } else if (e->dstate == DS_SHARED) {
      if (de_has(e, rq) && de_num(C, e) == 1) {               /* upgrade: the requester is the lone sharer */
        de_set_owner(C, e, (int32_t)rq);
        e->dstate = DS_MODIFIED;
        c_send(C, home, rq, GG_MSG_UPGRADE_REP, rq, addr, *t);
        completed = 1;
      } else {
        for (uint32_t w = 0; w < C->sharer_words; ++w)
          for (uint64_t b = e->sharers[w]; b; b &= b - 1)
            c_send(C, home, w * 64 + (uint32_t)__builtin_ctzll(b), M_INV_REQ, rq, addr, *t);
      }
    } else {                                                  /* UNCACHED */
      if (de_num(C, e) != 0) C->err = 1;
      info.loc = GG_LOC_L1D;                                  /* setCachingComponent(L1_DCACHE) */
      de_add(C, e, rq);
      de_set_owner(C, e, (int32_t)rq);
      e->dstate = DS_MODIFIED;
      sh_read_and_send(C, home, M_EX_REP, addr, data, rq, *t);
      completed = 1;
    }
  } else {
    c_send(C, home, c_home(C, addr), GG_MSG_DRAM_FETCH_REQ, rq, addr, *t);   /* fetchDataFromDram (:907-914) */
  }
  if (completed) {
    sh_set_info(C, home, addr, &info, e);
    sh_next(C, home, addr, t);
  }
}

/* processShReqFromL1Cache (:564-697) */
static void sh_process_sh(oracle_coh* C, uint32_t home, c_req* req, int data, int first, uint64_t* t)
{
  const uint64_t addr = req->addr;
  const uint32_t rq = req->requester;
  o_line info; c_dentry* e;
  sh_get_info(C, home, addr, M_SH_REQ, first, &info, &e, t);
  if (info.cstate == CS_I || !e) { C->err = 1; return; }
  int completed = 0;
  if (info.cstate != CS_DATA_INVALID) {
    if (e->dstate == DS_MODIFIED) {                           /* (MESI: DOWNGRADE_REQ to the exclusive owner) */
      c_send(C, home, (uint32_t)e->owner, C->mesi ? GG_MSG_DOWNGRADE_REQ : M_WB_REQ, rq, addr, *t);
    } else if (e->dstate == DS_SHARED) {
      de_add(C, e, rq);                                       /* full map: always added */
      sh_read_and_send(C, home, M_SH_REP, addr, data, rq, *t);
      completed = 1;
    } else {
      if (de_num(C, e) != 0) C->err = 1;
      info.loc = GG_LOC_L1D;
      de_add(C, e, rq);
      if (C->mesi) {                                          /* …sh_l2_mesi/l2_cache_cntlr.cc:671-687: an L1-D reader owns it EXCLUSIVE */
        e->dstate = DS_MODIFIED;
        de_set_owner(C, e, (int32_t)rq);
        sh_read_and_send(C, home, GG_MSG_SH_REP_EX, addr, data, rq, *t);
      } else {
        e->dstate = DS_SHARED;
        sh_read_and_send(C, home, M_SH_REP, addr, data, rq, *t);
      }
      completed = 1;
    }
  } else {
    c_send(C, home, c_home(C, addr), GG_MSG_DRAM_FETCH_REQ, rq, addr, *t);
  }
  if (completed) {
    sh_set_info(C, home, addr, &info, e);
    sh_next(C, home, addr, t);
  }
}

/* restartShmemReq (:813-847) */
static void sh_restart(oracle_coh* C, uint32_t home, c_req* req, const c_dentry* e, int data, uint64_t* t)
{
  *t += lat_to_ps(1, C->cfg.frequency_ghz);
  if (req->time < *t) req->time = *t;
  if (*t < req->time) *t = req->time;
  const uint32_t ds = e ? e->dstate : DS_UNCACHED;
  if (req->type == M_EX_REQ) { if (ds == DS_UNCACHED) sh_process_ex(C, home, req, data, 0, t); }
  else if (req->type == M_SH_REQ) sh_process_sh(C, home, req, data, 0, t);
  else if (req->type == M_NULLIFY_REQ) { if (ds == DS_UNCACHED) sh_process_nullify(C, home, req, data, t); }
  else C->err = 1;
}

/* L1CacheCntlr::insertCacheLine (l1_cache_cntlr.cc:230-274): an eviction goes to its L2 home */
static void sh_l1_insert(oracle_coh* C, uint32_t tile, uint64_t addr, uint32_t cstate, uint64_t t)
{
  c_tile* Tl = &C->t[tile];
  o_line in = { o_tag(&Tl->c.l1, addr), cstate, GG_LOC_INVALID };
  o_line ev = o_default_line();
  int eviction = 0; uint64_t ev_addr = 0;
  if (o_insert_line(&Tl->c.l1, addr, &in, &eviction, &ev_addr, &ev)) { C->err = 1; return; }
  if (!eviction) return;
  if (ev.cstate == CS_M) c_send(C, tile, c_home(C, ev_addr), M_FLUSH_REP, tile, ev_addr, t);
  else if (ev.cstate == CS_S || (C->mesi && ev.cstate == GG_CSTATE_EXCLUSIVE))
    c_send(C, tile, c_home(C, ev_addr), M_INV_REP, tile, ev_addr, t);
  else C->err = 1;
}
/* MESI operationPermissibleinL1Cache (…sh_l2_mesi/l1_cache_cntlr.cc:168-211): a
 * hit rewrites the line's info, MODIFIED on a write (an EXCLUSIVE line upgrades silently) */
static void sh_mesi_hit(oracle_coh* C, uint32_t tile, uint64_t addr, int is_write, o_line* info)
{
  if (is_write) info->cstate = CS_M;
  if (o_set_line_info(&C->t[tile].c.l1, addr, info)) C->err = 1;
}
/* L1CacheCntlr::invalidateCacheLine (:276-287) */
static void sh_l1_invalidate(oracle_coh* C, uint32_t tile, uint64_t addr)
{
  o_cache* l1 = &C->t[tile].c.l1;
  o_line info = o_default_line();
  o_get_line_info(l1, addr, &info);
  info.tag = O_INVALID_TAG; info.cstate = CS_I;
  if (o_set_line_info(l1, addr, &info)) C->err = 1;
}

/* The core's access (processMemOpFromCore, l1_cache_cntlr.cc:80-144): no L1
 * invalidate before a miss, the request (handleMsgFromCore, :289-302, at
 * once) straight to the line's L2 home */
static void sh_app_access(oracle_coh* C, uint32_t tile, uint64_t addr, int is_write, uint64_t s)
{
  c_tile* Tl = &C->t[tile];
  uint64_t t = s;
  o_line info = o_default_line();
  o_get_line_info(&Tl->c.l1, addr, &info);                    /* operationPermissibleinL1Cache (:169-204) */
  const int hit = is_write ? cs_writable(info.cstate) : cs_readable(info.cstate);
  if (hit && C->mesi) sh_mesi_hit(C, tile, addr, is_write, &info);
  o_update_miss_counters(&Tl->c.l1, addr, is_write, !hit);
  if (hit) {
    t += C->lat_l1_data;
    if (o_access_line(&Tl->c.l1, addr, is_write)) C->err = 1;  /* accessCache (:146-167) */
    c_finish_access(C, tile, s, t, GG_LVL_L1);
    return;
  }
  t += C->lat_l1_tags;
  if (Tl->out_addr != C_INVALID_ADDR) C->err = 1;
  Tl->out_addr = addr; Tl->out_time = t;
  c_send(C, tile, c_home(C, addr), is_write ? M_EX_REQ : M_SH_REQ, tile, addr, t);
  Tl->blocked = 1;
  Tl->pend_start = s;
}

/* MemoryManager::handleMsgFromNetwork (…sh_l2_msi/memory_manager.cc:215-294):
 * the L1 (replies and requests from the L2), the L2 slice (requests and
 * replies from L1s, DRAM replies) and the DRAM controller */
static void sh_handle(oracle_coh* C, uint32_t tile, const gg_cmsg* m)
{
  c_tile* Tl = &C->t[tile];
  uint64_t t = m->arrival_ps;
  const uint64_t addr = m->addr;
  const uint32_t sender = m->src;
  switch (m->type) {
  /* ---- L1CacheCntlr::handleMsgFromL2Cache (l1_cache_cntlr.cc:304-362) */
  case M_EX_REP: case M_SH_REP: case GG_MSG_UPGRADE_REP: case GG_MSG_SH_REP_EX: {
    if (!Tl->blocked || Tl->out_addr != addr) { C->err = 1; return; }
    if (m->type == GG_MSG_UPGRADE_REP) {                           /* processUpgradeRepFromL2Cache (:388-409) */
      o_line l1i = o_default_line();
      o_get_line_info(&Tl->c.l1, addr, &l1i);
      if (l1i.cstate != CS_S) C->err = 1;
      l1i.cstate = CS_M;
      if (o_set_line_info(&Tl->c.l1, addr, &l1i)) C->err = 1;
    } else {
      sh_l1_insert(C, tile, addr, m->type == M_EX_REP ? CS_M : m->type == GG_MSG_SH_REP_EX ? GG_CSTATE_EXCLUSIVE : CS_S, t);
    }
    if (Tl->out_time > t) C->err = 1;
    t += C->lat_l1_data;                                      /* incrCurrTime(L1, ACCESS_DATA_AND_TAGS) */
    Tl->out_addr = C_INVALID_ADDR;
    /* wakeUpAppThread: the core's second attempt (access_num == 2, :97-119) */
    const int is_write = (int)(C->meta[Tl->rec] & GG_META_WRITE);
    o_line info = o_default_line();
    o_get_line_info(&Tl->c.l1, addr, &info);
    if (!(is_write ? cs_writable(info.cstate) : cs_readable(info.cstate))) { C->err = 1; return; }
    if (C->mesi) sh_mesi_hit(C, tile, addr, is_write, &info);
    t += C->lat_l1_data;
    if (o_access_line(&Tl->c.l1, addr, is_write)) C->err = 1;
    Tl->blocked = 0;
    c_finish_access(C, tile, Tl->pend_start, t, GG_LVL_DIR);
    break;
  }
  case M_INV_REQ: {                                           /* processInvReqFromL2Cache (:411-448) */
    o_line l1i = o_default_line();
    o_get_line_info(&Tl->c.l1, addr, &l1i);
    if (C->mesi) {                                            /* …sh_l2_mesi/l1:432-498: a MODIFIED line is flushed */
      if (l1i.cstate == CS_M) {
        t += C->lat_l1_data;
        if (o_access_line(&Tl->c.l1, addr, 0)) C->err = 1;   /* readCacheLine */
        sh_l1_invalidate(C, tile, addr);
        c_send(C, tile, sender, M_FLUSH_REP, m->requester, addr, t);
      } else if (l1i.cstate != CS_I) {
        t += C->lat_l1_tags;
        if (l1i.cstate != CS_S && l1i.cstate != GG_CSTATE_EXCLUSIVE) C->err = 1;
        sh_l1_invalidate(C, tile, addr);
        c_send(C, tile, sender, M_INV_REP, m->requester, addr, t);
      } else {
        t += C->lat_l1_tags;
      }
      break;
    }
    t += C->lat_l1_tags;
    if (l1i.cstate != CS_I) {
      if (l1i.cstate != CS_S) C->err = 1;
      sh_l1_invalidate(C, tile, addr);
      c_send(C, tile, sender, M_INV_REP, m->requester, addr, t);
    }
    break;
  }
  case M_FLUSH_REQ:                                           /* processFlushReqFromL2Cache (:450-489) */
  case M_WB_REQ: {                                            /* processWbReqFromL2Cache (:491-536) */
    o_line l1i = o_default_line();
    o_get_line_info(&Tl->c.l1, addr, &l1i);
    if (l1i.cstate != CS_I) {
      if (l1i.cstate != CS_M) C->err = 1;
      t += C->lat_l1_data;
      if (o_access_line(&Tl->c.l1, addr, 0)) C->err = 1;     /* readCacheLine */
      if (m->type == M_FLUSH_REQ) {
        sh_l1_invalidate(C, tile, addr);
        c_send(C, tile, sender, M_FLUSH_REP, m->requester, addr, t);
      } else {
        l1i.cstate = CS_S;
        if (o_set_line_info(&Tl->c.l1, addr, &l1i)) C->err = 1;
        c_send(C, tile, sender, M_WB_REP, m->requester, addr, t);
      }
    } else {
      t += C->lat_l1_tags;
    }
    break;
  }
  case GG_MSG_DOWNGRADE_REQ: {                                /* MESI processDowngradeReqFromL2Cache (…sh_l2_mesi/l1:540-600) */
    o_line l1i = o_default_line();
    o_get_line_info(&Tl->c.l1, addr, &l1i);
    if (l1i.cstate != CS_I) {
      if (l1i.cstate == CS_M) {
        t += C->lat_l1_data;
        if (o_access_line(&Tl->c.l1, addr, 0)) C->err = 1;   /* readCacheLine */
        c_send(C, tile, sender, M_WB_REP, m->requester, addr, t);
      } else {
        if (l1i.cstate != GG_CSTATE_EXCLUSIVE) C->err = 1;
        t += C->lat_l1_tags;
        c_send(C, tile, sender, GG_MSG_DOWNGRADE_REP, m->requester, addr, t);
      }
      l1i.cstate = CS_S;
      if (o_set_line_info(&Tl->c.l1, addr, &l1i)) C->err = 1;
    } else {
      t += C->lat_l1_tags;
    }
    break;
  }
  /* ---- L2CacheCntlr::handleMsgFromL1Cache (l2_cache_cntlr.cc:191-276) */
  case M_EX_REQ: case M_SH_REQ: {
    t += C->lat_l2_data;                                      /* every message into the L2 */
    c_req r; memset(&r, 0, sizeof(r));
    r.addr = addr; r.time = t; r.type = m->type; r.requester = m->requester;
    c_req* p = rq_enqueue(Tl, r);
    if (rq_count(Tl, addr) == 1) {
      if (m->type == M_EX_REQ) sh_process_ex(C, tile, p, SH_NULL_DATA, 1, &t);
      else sh_process_sh(C, tile, p, SH_NULL_DATA, 1, &t);
    }
    break;
  }
  case M_INV_REP: case M_FLUSH_REP: case M_WB_REP: case GG_MSG_DOWNGRADE_REP: {
    t += C->lat_l2_data;
    o_line info; c_dentry* e;
    sh_get_info(C, tile, addr, m->type, 0, &info, &e, &t);
    if (info.tag == O_INVALID_TAG || !e) { C->err = 1; return; }
    if (m->type == M_INV_REP) {                               /* processInvRepFromL1Cache (:699-729) */
      if (e->dstate == DS_SHARED) {
        de_remove(C, e, sender);
        if (de_num(C, e) == 0) e->dstate = DS_UNCACHED;
      } else if (C->mesi && e->dstate == DS_MODIFIED) {       /* …sh_l2_mesi/l2:739-751: the exclusive owner */
        if (de_num(C, e) != 1) C->err = 1;
        de_remove(C, e, sender);
        de_set_owner(C, e, C_INVALID_TILE);
        e->dstate = DS_UNCACHED;
      }
    } else if (m->type == GG_MSG_DOWNGRADE_REP) {             /* processDowngradeRepFromL1Cache (…sh_l2_mesi/l2:804-836) */
      if (e->dstate == DS_MODIFIED) {
        de_set_owner(C, e, C_INVALID_TILE);
        e->dstate = DS_SHARED;
      }
    } else if (m->type == M_FLUSH_REP) {                      /* processFlushRepFromL1Cache (:731-773) */
      if (e->dstate == DS_MODIFIED) {
        c_req* f = rq_front(Tl, addr);
        if (!f || f->type == M_SH_REQ) sh_cache_access(C, Tl, addr, 1);   /* writeCacheLine */
        info.cstate = CS_DIRTY;
        de_remove(C, e, sender);
        de_set_owner(C, e, C_INVALID_TILE);
        e->dstate = DS_UNCACHED;
      }
    } else {                                                  /* processWbRepFromL1Cache (:775-811) */
      if (e->dstate == DS_MODIFIED) {
        sh_cache_access(C, Tl, addr, 1);
        info.cstate = CS_DIRTY;
        de_set_owner(C, e, C_INVALID_TILE);
        e->dstate = DS_SHARED;
      }
    }
    sh_set_info(C, tile, addr, &info, e);
    c_req* f = rq_front(Tl, addr);
    if (f) sh_restart(C, tile, f, e, m->type != M_INV_REP && m->type != GG_MSG_DOWNGRADE_REP, &t);
    break;
  }
  /* ---- L2CacheCntlr::handleMsgFromDram (:278-303) */
  case GG_MSG_DRAM_FETCH_REP: {
    t += C->lat_l2_data;
    o_line info = o_default_line(); c_dentry* e = NULL;
    sh_cache_get(C, Tl, addr, &info, &e);
    c_req* f = rq_front(Tl, addr);
    if (!f || !e) { C->err = 1; return; }
    if (f->type == M_SH_REQ) sh_cache_access(C, Tl, addr, 1);  /* writeCacheLine */
    else if (f->type != M_EX_REQ) C->err = 1;
    info.cstate = CS_CLEAN;
    sh_set_info(C, tile, addr, &info, e);
    sh_restart(C, tile, f, e, 1, &t);
    break;
  }
  /* ---- DramCntlr::handleMsgFromL2Cache (…sh_l2_msi/dram_cntlr.cc:19-52) */
  case GG_MSG_DRAM_FETCH_REQ:
    dram_get(C, Tl, &t);                                      /* getDataFromDram: the access latency */
    c_send(C, tile, sender, GG_MSG_DRAM_FETCH_REP, m->requester, addr, t);
    break;
  case GG_MSG_DRAM_STORE_REQ:
    dram_put(C, Tl, t);                                       /* putDataToDram */
    break;
  default: C->err = 1;
  }
}

/* ---- the canonical schedule ----------------------------------------------- */
static int cmsg_chan_lt(const gg_cmsg* a, const gg_cmsg* b)
{
  return a->src < b->src || (a->src == b->src && a->seq < b->seq);
}
static int cmp_chan(const void* x, const void* y)
{
  const gg_cmsg* a = (const gg_cmsg*)x; const gg_cmsg* b = (const gg_cmsg*)y;
  return cmsg_chan_lt(a, b) ? -1 : (cmsg_chan_lt(b, a) ? 1 : 0);
}

/* Handle the tile's inbox: per-channel FIFO, channels merged by (arrival, sender). */
static void c_drain_inbox(oracle_coh* C, uint32_t tile)
{
  c_tile* Tl = &C->t[tile];
  uint64_t n = Tl->nin;
  if (!n) return;
  gg_cmsg* in = (gg_cmsg*)malloc(sizeof(gg_cmsg) * n);
  memcpy(in, Tl->in, sizeof(gg_cmsg) * n);
  Tl->nin = 0;
  qsort(in, n, sizeof(gg_cmsg), cmp_chan);
  /* channel heads: the first message of each run of equal src */
  uint64_t* head = (uint64_t*)malloc(sizeof(uint64_t) * n);
  uint64_t* end = (uint64_t*)malloc(sizeof(uint64_t) * n);
  uint64_t nch = 0;
  for (uint64_t i = 0; i < n; ++i) {
    if (i == 0 || in[i].src != in[i - 1].src) { head[nch] = i; end[nch] = i; nch++; }
    end[nch - 1] = i + 1;
  }
  for (uint64_t k = 0; k < n; ++k) {
    uint64_t best = ~0ull;
    for (uint64_t c = 0; c < nch; ++c) {
      if (head[c] == end[c]) continue;
      if (best == ~0ull) { best = c; continue; }
      const gg_cmsg* a = &in[head[c]]; const gg_cmsg* b = &in[head[best]];
      if (a->arrival_ps < b->arrival_ps || (a->arrival_ps == b->arrival_ps && a->src < b->src)) best = c;
    }
    const gg_cmsg* m = &in[head[best]++];
    Tl->st[GG_CT_MSGS_RECEIVED]++;
    if (C->shl2) sh_handle(C, tile, m);
    else if (msg_to_directory(m->type)) { if (C->mosi) mo_dd_handle(C, tile, m); else dd_handle(C, tile, m); }
    else if (C->mosi) mo_l2_handle(C, tile, m);
    else l2c_handle(C, tile, m);
  }
  free(head); free(end); free(in);
}

/* Run the tile's trace until it blocks or the next access starts at or after the barrier. */
static void c_run_app(oracle_coh* C, uint32_t tile, uint64_t barrier)
{
  c_tile* Tl = &C->t[tile];
  while (!Tl->blocked && Tl->rec < Tl->rec_end) {
    uint32_t meta = C->meta[Tl->rec];
    if (meta == GG_META_BARRIER) {               /* SyncClient::barrierWait at the core's time (sync_client.cc:265-281) */
      if (Tl->clk < barrier) Tl->blocked = C_BAR_WAIT;
      return;
    }
    uint64_t s = Tl->clk + (uint64_t)((meta & 0x7FFFFFFFu) >> 1) * C->gap_ps;
    if (s >= barrier && !(meta & GG_META_CONT)) return;   /* a multi-line access is one instruction */
    const uint64_t a = C->addr[Tl->rec] & ~((uint64_t)C->cfg.line_size - 1);
    if (C->shl2) sh_app_access(C, tile, a, (int)(meta & GG_META_WRITE), s);
    else c_app_access(C, tile, a, (int)(meta & GG_META_WRITE), s);
  }
}

static void c_deliver(oracle_coh* C, const gg_cmsg* m)
{
  c_tile* D = &C->t[m->dst];
  D->in = (gg_cmsg*)grow(D->in, &D->capin, D->nin + 1, sizeof(gg_cmsg));
  D->in[D->nin++] = *m;
}

static int cmp_send(const void* x, const void* y)
{
  const gg_cmsg* a = (const gg_cmsg*)x; const gg_cmsg* b = (const gg_cmsg*)y;
  if (a->send_ps != b->send_ps) return a->send_ps < b->send_ps ? -1 : 1;
  return cmp_chan(x, y);
}

static void c_hold(oracle_coh* C, const gg_cmsg* m)
{
  C->bnd = (gg_cmsg*)grow(C->bnd, &C->capbnd, C->nbnd + 1, sizeof(gg_cmsg));
  C->bnd[C->nbnd++] = *m;
  C->ri[GG_RI_BOUNDARY_MSGS]++;
}

/* Route the step's messages (NetworkModel, memory network) and deliver them.
 * emesh_hop_by_hop routes the held packets resuming this step (the first of a
 * quantum) in the same batch; a packet whose next router lies in another
 * logical shard is held for the quantum boundary (noc_hbh_walk). */
static uint64_t c_nsent(const oracle_coh* C)
{
  uint64_t n = C->nstep;
  for (int i = 1; i < C->nthreads; ++i) n += C->tnstep[i];
  return n;
}
static void c_route_step(oracle_coh* C)
{
  uint64_t n = c_nsent(C) + C->nres;
  if (!n) return;
  gg_cmsg* B = (gg_cmsg*)malloc(sizeof(gg_cmsg) * n);
  uint64_t o = C->nstep;
  memcpy(B, C->step, sizeof(gg_cmsg) * C->nstep);
  for (int i = 1; i < C->nthreads; ++i) {
    if (C->tnstep[i]) memcpy(B + o, C->tstep[i], sizeof(gg_cmsg) * C->tnstep[i]);
    o += C->tnstep[i]; C->tnstep[i] = 0;
  }
  if (C->nres) memcpy(B + o, C->res, sizeof(gg_cmsg) * C->nres);
  C->nstep = 0; C->nres = 0;
  /* canonical batch order for the router queues: (send time, sender, sequence) */
  qsort(B, n, sizeof(gg_cmsg), cmp_send);
  uint32_t* src = (uint32_t*)malloc(4 * n); uint32_t* dst = (uint32_t*)malloc(4 * n);
  uint32_t* len = (uint32_t*)malloc(4 * n); uint32_t* cur = (uint32_t*)malloc(4 * n);
  uint64_t* tm = (uint64_t*)malloc(8 * n); uint64_t* arr = (uint64_t*)malloc(8 * n);
  uint64_t* zl = (uint64_t*)malloc(8 * n); uint64_t* ct = (uint64_t*)malloc(8 * n);
  uint8_t* inj = (uint8_t*)malloc(n); uint8_t* held = (uint8_t*)calloc(n, 1);
  for (uint64_t k = 0; k < n; ++k) {
    const gg_cmsg* m = &B[k];
    src[k] = m->src; dst[k] = m->dst; tm[k] = m->send_ps;
    len[k] = msg_has_data(m->type) ? C->bits_data : m->type == GG_MSG_INV_FLUSH_COMBINED_REQ ? C->bits_ifc : C->bits_req;
    if (m->hop == GG_HOP_NONE) { inj[k] = 1; cur[k] = m->src; arr[k] = m->send_ps; zl[k] = 0; ct[k] = 0; }
    else { inj[k] = 0; cur[k] = m->hop; arr[k] = m->arrival_ps; zl[k] = m->zero_load_ps;
           ct[k] = m->arrival_ps - m->send_ps - m->zero_load_ps; }
  }
  if (C->cfg.net_model == GG_NET_EMESH_HOP_BY_HOP) {
    if (C->noc->n != C->noc->w * C->noc->h) C->err = 1;
    else if (C->nthreads > 1)
      noc_hbh_walk_par(C->noc, n, src, dst, len, cur, arr, zl, ct, inj, C->K > 1 ? C->shard : NULL, held, C->nthreads);
    else noc_hbh_walk(C->noc, n, src, dst, len, cur, arr, zl, ct, inj, C->K > 1 ? C->shard : NULL, held);
  } else if (oracle_noc_route(C->noc, n, src, dst, len, tm, arr, zl, ct)) C->err = 1;
  for (uint64_t k = 0; k < n; ++k) {
    gg_cmsg* m = &B[k];
    if (inj[k]) { if (m->src == m->dst) C->ri[GG_RI_SELF_MSGS]++; else C->ri[GG_RI_NET_MSGS]++; }
    m->arrival_ps = arr[k]; m->zero_load_ps = zl[k];
    if (held[k]) { m->hop = cur[k]; c_hold(C, m); continue; }
    m->hop = GG_HOP_NONE;
    if (c_shard(C, m->src) == c_shard(C, m->dst) || C->cfg.net_model == GG_NET_EMESH_HOP_BY_HOP) c_deliver(C, m);
    else c_hold(C, m);
  }
  free(B); free(src); free(dst); free(len); free(cur); free(tm); free(arr); free(zl); free(ct); free(inj); free(held);
}

/* A record of the quantum boundary for an owned tile: a message into the
 * inbox of its receiver, or a held packet resuming at router `hop`. */
static int c_accept(oracle_coh* C, const gg_cmsg* m)
{
  const uint32_t at = m->hop == GG_HOP_NONE ? m->dst : m->hop;
  if (at >= C->T || m->dst >= C->T || !c_owned(C, at)) return GG_ERR_INVALID;
  if (m->hop == GG_HOP_NONE) { c_deliver(C, m); return 0; }
  C->res = (gg_cmsg*)grow(C->res, &C->capres, C->nres + 1, sizeof(gg_cmsg));
  C->res[C->nres++] = *m;
  return 0;
}

/* ---- public API ----------------------------------------------------------- */
oracle_coh* oracle_coh_create(const gg_config* cfg)
{
  oracle_coh* C = (oracle_coh*)calloc(1, sizeof(*C));
  C->cfg = *cfg;
  C->T = cfg->num_tiles;
  C->K = cfg->num_shards ? cfg->num_shards : 1;
  C->k0 = cfg->shard_begin;
  C->k1 = cfg->shard_end ? cfg->shard_end : C->K;
  const double f = cfg->frequency_ghz;
  /* CachePerfModelParallel::getLatency (cache_perf_model_parallel.h:14-29) */
  C->lat_l1_data = lat_to_ps(cfg->l1d_data_cycles, f);
  C->lat_l1_tags = lat_to_ps(cfg->l1d_tags_cycles, f);
  C->lat_l2_data = lat_to_ps(cfg->l2_data_cycles, f);
  C->lat_l2_tags = lat_to_ps(cfg->l2_tags_cycles, f);
  C->gap_ps = lat_to_ps(1, f);                   /* ONE_CYCLE per non-memory instruction (synthetic_memory.cc:158-163) */
  C->quantum_ps = (uint64_t)cfg->quantum_ns * 1000ull;
  /* DirectoryCache sizing (directory_cache.cc:46-90, 243-322) */
  C->dir_assoc = cfg->dir_assoc;
  uint32_t slices = C->T;                        /* dram/num_controllers = ALL */
  uint32_t entries;
  if (cfg->dir_total_entries == 0) {
    uint32_t sets = (uint32_t)ceil(2.0 * cfg->l2_size_kb * 1024 * C->T / (64.0 * cfg->dir_assoc * slices));
    sets = 1u << ceil_log2(sets);
    entries = sets * cfg->dir_assoc;
  } else entries = cfg->dir_total_entries;
  C->dir_sets = entries / cfg->dir_assoc;
  C->log_dir_sets = (uint32_t)floor_log2(C->dir_sets);
  if (C->dir_sets < 2) C->err = 1;               /* one set: computeSetIndex folds 0-bit fields and never ends */
  C->log_slices = (uint32_t)ceil_log2(slices);
  C->log_line = (uint32_t)floor_log2(cfg->line_size);
  uint32_t entry_bytes = (uint32_t)ceil(1.0 * C->T / 8);   /* DirectoryEntry::getSize(FULL_MAP) = app tiles bits */
  uint64_t dir_size = (uint64_t)entries * entry_bytes;
  uint64_t cyc = cfg->dir_access_cycles;
  if (cyc == 0) {
    uint32_t kb = (uint32_t)ceil(1.0 * dir_size / 1024);
    cyc = kb <= 16 ? 1 : kb <= 32 ? 2 : kb <= 64 ? 4 : kb <= 128 ? 6 : kb <= 256 ? 8 :
          kb <= 512 ? 10 : kb <= 1024 ? 13 : kb <= 2048 ? 16 : 20;
  }
  C->lat_dir = lat_to_ps(cyc, f);
  C->sharer_words = (C->T + 63) / 64;
  /* network_model.cc:185-200 + shmem_msg.cc:100-125 */
  uint32_t idb = C->T > 1 ? (uint32_t)ceil_log2(C->T) : 0;
  C->bits_req = 2 * idb + 4 + 48;
  C->bits_data = C->bits_req + 8 * cfg->line_size;
  C->bits_ifc = C->bits_req + idb;               /* …mosi/shmem_msg.cc:137-139: + single receiver */
  C->mosi = cfg->protocol == GG_PROTO_MOSI;
  C->shl2 = cfg->protocol == GG_PROTO_SHL2_MSI || cfg->protocol == GG_PROTO_SHL2_MESI;
  C->mesi = cfg->protocol == GG_PROTO_SHL2_MESI;
  if (cfg->protocol > GG_PROTO_SHL2_MESI) C->err = 1;
  if (C->shl2 && cfg->l2_track_miss_types) C->err = 1;           /* (the slice's miss types are not restated) */
  C->dram_proc = (uint64_t)((float)cfg->line_size / cfg->dram_bandwidth) + 1;  /* dram_perf_model.cc:48,92 */
  C->dram_cost = (uint64_t)(float)cfg->dram_latency_ns;
  C->noc = oracle_noc_create(cfg);
  C->shard = (uint32_t*)calloc(C->T ? C->T : 1, sizeof(uint32_t));
  if (oracle_shard_map(C->T, C->K, C->shard)) C->err = 1;
  C->t = (c_tile*)calloc(C->T, sizeof(c_tile));
  for (uint32_t i = 0; i < C->T; ++i) {
    c_tile* Tl = &C->t[i];
    if (C->err || !c_owned(C, i)) continue;          /* tiles of other shards: no state here */
    /* the L1-D is write-through under pr_l1_pr_l2 (l1_cache_cntlr.cc:59), write-back under sh_l2 (…sh_l2_msi/l1_cache_cntlr.cc:57) */
    o_cache_init(&Tl->c.l1, cfg->l1d_size_kb, cfg->l1d_assoc, cfg->line_size, cfg->l1d_policy, C->shl2);
    o_cache_init(&Tl->c.l2, cfg->l2_size_kb, cfg->l2_assoc, cfg->line_size, cfg->l2_policy, 1);
    /* MSI: the L1-D takes the L1-I flag (l1_cache_cntlr.cc:69); MOSI its own (…mosi/l1_cache_cntlr.cc:68) */
    Tl->c.l1.track = ((C->mosi || C->shl2) ? cfg->l1d_track_miss_types : cfg->l1i_track_miss_types) != 0;   /* sh_l2: …sh_l2_msi/l1:67 */
    Tl->c.l2.track = cfg->l2_track_miss_types != 0;
    Tl->out_addr = C_INVALID_ADDR;
    Tl->slot = (c_dentry**)calloc((size_t)entries, sizeof(c_dentry*));   /* entries: dc_slot */
    if (C->shl2) {
      Tl->sde = (c_dentry**)calloc((size_t)Tl->c.l2.sets * Tl->c.l2.ways, sizeof(c_dentry*));
      C->log_l2_sets = (uint32_t)floor_log2(Tl->c.l2.sets);
    }
    if (cfg->dram_queue_model_enabled)
      Tl->dram_q = oracle_qmodel_create(cfg->dram_queue_model_type, qm_aux_of(cfg, cfg->dram_queue_model_type),
                                        C->dram_proc, (int)cfg->max_list_size, (int)cfg->analytical_enabled);
  }
  return C;
}

void oracle_coh_destroy(oracle_coh* C)
{
  if (!C) return;
  uint32_t entries = C->dir_sets * C->dir_assoc;
  for (uint32_t i = 0; i < C->T; ++i) {
    c_tile* Tl = &C->t[i];
    o_cache_free(&Tl->c.l1); o_cache_free(&Tl->c.l2);
    if (Tl->slot) for (uint32_t e = 0; e < entries; ++e) de_free(Tl->slot[e]);
    for (uint32_t e = 0; e < Tl->nreplaced; ++e) de_free(Tl->replaced[e]);
    for (uint32_t e = 0; e < Tl->nq; ++e) free(Tl->q[e]);
    if (Tl->sde) for (size_t e = 0; e < (size_t)Tl->c.l2.sets * Tl->c.l2.ways; ++e) de_free(Tl->sde[e]);
    for (uint32_t e = 0; e < Tl->nev; ++e) de_free(Tl->evd[e]);
    free(Tl->sde); free(Tl->eva); free(Tl->evl); free(Tl->evd);
    free(Tl->slot); free(Tl->replaced); free(Tl->q); free(Tl->in); free(Tl->cdl);
    oracle_htree_destroy(Tl->dram_q);
  }
  oracle_noc_destroy(C->noc);
  for (int i = 1; i < C->nthreads; ++i) free(C->tstep[i]);
  free(C->tstep); free(C->tnstep); free(C->tcapstep);
  free(C->t); free(C->step); free(C->bnd); free(C->res); free(C->shard); free(C);
}

int oracle_coh_begin(oracle_coh* C, const uint64_t* addr, const uint32_t* meta,
                     const uint64_t* tile_offsets, uint64_t* access_out)
{
  if (C->err) return GG_ERR_INVALID;
  C->addr = addr; C->meta = meta; C->out = access_out;
  C->has_barrier = 0;
  for (uint32_t i = 0; i < C->T; ++i) {
    C->t[i].rec = tile_offsets[i];
    C->t[i].rec_end = c_owned(C, i) ? tile_offsets[i + 1] : tile_offsets[i];
    for (uint64_t r = tile_offsets[i]; r < tile_offsets[i + 1]; ++r)
      if (meta[r] == GG_META_BARRIER) C->has_barrier = 1;
  }
  return 0;
}

/* One quantum on the owned shards; status = {steps, boundary msgs, min next start, active, blocked}. */
int oracle_coh_quantum(oracle_coh* C, uint64_t q, uint64_t* status)
{
  if (C->has_barrier && !C->in_run) return GG_ERR_UNSUPPORTED;   /* barriers: oracle_coh_run only */
  const uint64_t barrier = (q + 1) * C->quantum_ps;
  uint64_t steps = 0;
  for (;;) {
    if (C->nthreads > 1) {
      /* a step's tiles touch only their own state (a home's directory and DRAM
       * queue are the home tile's); what they send is routed after the step */
#pragma omp parallel for num_threads(C->nthreads) schedule(dynamic, 8)
      for (uint32_t i = 0; i < C->T; ++i) {
        if (!c_owned(C, i)) continue;
        c_drain_inbox(C, i);
        c_run_app(C, i, barrier);
      }
    } else {
      for (uint32_t i = 0; i < C->T; ++i) {
        if (!c_owned(C, i)) continue;
        c_drain_inbox(C, i);
        c_run_app(C, i, barrier);
      }
    }
    ++steps;
    if (c_nsent(C) == 0 && C->nres == 0) break;
    c_route_step(C);
    if (C->err) break;
  }
  C->ri[GG_RI_STEPS] += steps;
  C->ri[GG_RI_QUANTA]++;
  C->ri[GG_RI_FINAL_QUANTUM] = q;
  uint64_t mn = ~0ull, active = 0, blocked = 0;
  for (uint32_t i = 0; i < C->T; ++i) {
    c_tile* Tl = &C->t[i];
    if (!c_owned(C, i) || Tl->rec >= Tl->rec_end) continue;
    active++;
    if (Tl->blocked == C_BAR_WAIT) continue;     /* waits for the other tiles, not for time */
    if (Tl->blocked) { blocked++; continue; }
    const uint32_t nm = C->meta[Tl->rec];         /* a BARRIER record is taken at the tile's clock */
    uint64_t s = Tl->clk + (nm == GG_META_BARRIER ? 0ull : (uint64_t)((nm & 0x7FFFFFFFu) >> 1)) * C->gap_ps;
    if (s < mn) mn = s;
  }
  status[0] = steps; status[1] = C->nbnd; status[2] = mn; status[3] = active; status[4] = blocked;
  return C->err ? GG_ERR_STATE : 0;
}

/* Tile-parallel steps on `threads` OpenMP threads (the all-core CPU
 * baseline): the tiles of a step, then the routing stages of
 * noc_hbh_walk_par, in parallel; every output equals the serial run's. */
int oracle_coh_set_threads(oracle_coh* C, int threads)
{
  if (threads < 1) threads = 1;
  for (int i = 1; i < C->nthreads; ++i) free(C->tstep[i]);
  free(C->tstep); free(C->tnstep); free(C->tcapstep);
  C->nthreads = threads;
  C->tstep = (gg_cmsg**)calloc((size_t)threads, sizeof(gg_cmsg*));
  C->tnstep = (uint64_t*)calloc((size_t)threads, sizeof(uint64_t));
  C->tcapstep = (uint64_t*)calloc((size_t)threads, sizeof(uint64_t));
  return 0;
}

/* Take the held cross-shard messages (sorted by destination shard, then channel). */
static const uint32_t* cmp_dst_shard_map;
static uint32_t rec_shard(const uint32_t* map, const gg_cmsg* m) { return map[m->hop == GG_HOP_NONE ? m->dst : m->hop]; }
static int cmp_dst_shard(const void* x, const void* y)
{
  const gg_cmsg* a = (const gg_cmsg*)x; const gg_cmsg* b = (const gg_cmsg*)y;
  uint32_t sa = rec_shard(cmp_dst_shard_map, a), sb = rec_shard(cmp_dst_shard_map, b);
  if (sa != sb) return sa < sb ? -1 : 1;
  return cmp_chan(x, y);
}
uint64_t oracle_coh_export(oracle_coh* C, gg_cmsg* out, uint64_t cap)
{
  uint64_t n = C->nbnd;
  cmp_dst_shard_map = C->shard;
  qsort(C->bnd, n, sizeof(gg_cmsg), cmp_dst_shard);
  if (n > cap) return ~0ull;
  memcpy(out, C->bnd, sizeof(gg_cmsg) * n);
  C->nbnd = 0;
  return n;
}

int oracle_coh_import(oracle_coh* C, const gg_cmsg* in, uint64_t n)
{
  for (uint64_t i = 0; i < n; ++i)
    if (c_accept(C, &in[i])) return GG_ERR_INVALID;
  return 0;
}

/* The whole run on one process owning every shard. */
int oracle_coh_run(oracle_coh* C, const uint64_t* addr, const uint32_t* meta,
                   const uint64_t* tile_offsets, uint64_t* access_out)
{
  if (C->k0 != 0 || C->k1 != C->K) return GG_ERR_INVALID;
  int rc0 = oracle_coh_begin(C, addr, meta, tile_offsets, access_out);
  if (rc0) return rc0;
  uint64_t q = 0, st[5];
  C->in_run = 1;
  for (;;) {
    int rc = oracle_coh_quantum(C, q, st);
    if (rc) { C->in_run = 0; return rc; }
    uint64_t nb = C->nbnd;
    C->nbnd = 0;
    for (uint64_t i = 0; i < nb; ++i)                    /* the boundary exchange */
      if (c_accept(C, &C->bnd[i])) { C->in_run = 0; return GG_ERR_STATE; }
    if (st[3] == 0 && nb == 0) {                 /* every trace finished, nothing in flight */
      if (C->qhook) C->qhook(C->qhook_arg, q, q + 1);
      break;
    }
    const uint64_t q_ended = q;
    uint64_t bw = 0, bmax = 0;                   /* tiles waiting at a BARRIER record, latest arrival */
    for (uint32_t i = 0; i < C->T; ++i) {
      const c_tile* Tl = &C->t[i];
      if (Tl->rec < Tl->rec_end && Tl->blocked == C_BAR_WAIT) { bw++; if (Tl->clk > bmax) bmax = Tl->clk; }
    }
    if (nb == 0 && st[4] == 0 && bw && bw == st[3]) {
      /* every unfinished tile waits: SimBarrier::wait releases them all at
       * the latest arrival (sync_server.cc:133-170, 357-383), each core's
       * time advanced by the difference (sync_client.cc:306-314) */
      for (uint32_t i = 0; i < C->T; ++i) {
        c_tile* Tl = &C->t[i];
        if (Tl->rec >= Tl->rec_end || Tl->blocked != C_BAR_WAIT) continue;
        if (C->out) C->out[Tl->rec] = ((bmax - Tl->clk) << 2) | GG_LVL_SYNC;
        Tl->clk = bmax; Tl->rec++; Tl->blocked = 0;
        Tl->st[GG_CT_CLOCK_PS] = bmax;            /* the core clock after the release */
      }
      uint64_t nq = bmax / C->quantum_ps;
      q = nq > q + 1 ? nq : q + 1;
    } else if (nb == 0 && st[4] == 0) {          /* nothing in flight: skip empty quanta */
      uint64_t nq = st[2] / C->quantum_ps;
      q = nq > q + 1 ? nq : q + 1;
    } else if (nb == 0 && st[4] != 0) {
      return GG_ERR_STATE;                       /* blocked with nothing in flight: deadlock */
    } else {
      q = q + 1;
    }
    if (C->qhook) C->qhook(C->qhook_arg, q_ended, q);
  }
  C->in_run = 0;
  return C->err ? GG_ERR_STATE : 0;
}

/* A function oracle_coh_run calls between quanta: fn(arg, q, nq) when quantum
 * q has ended (its boundary records handed over, a BARRIER released) and
 * quantum nq runs next; after the last quantum nq = q + 1.  The state it may
 * read (counters, oracle_coh_census) is that after quantum q's last step: the
 * hand-over and the release change none of it.  NULL: none.  The series it
 * gives is checked against the stepped run (begin / quantum / export /
 * import) on traces without BARRIER records only: the stepped run takes no
 * others (tests/test_replication_census.py). */
void oracle_coh_set_quantum_hook(oracle_coh* C, void (*fn)(void*, uint64_t, uint64_t), void* arg)
{
  C->qhook = fn; C->qhook_arg = arg;
}

void oracle_coh_tile_stats(const oracle_coh* C, uint64_t* out)
{
  for (uint32_t i = 0; i < C->T; ++i)
    memcpy(out + (size_t)i * GG_NUM_TILE_STATS, C->t[i].st, sizeof(uint64_t) * GG_NUM_TILE_STATS);
  for (uint32_t i = 0; i < C->T; ++i) {
    if (!C->t[i].dram_q) continue;
    out[(size_t)i * GG_NUM_TILE_STATS + GG_CT_DRAM_QUEUE_ANALYTICAL] = oracle_htree_analytical_requests(C->t[i].dram_q);
    /* QueueModel utilization counters (queue_model.cc:49-55) */
    out[(size_t)i * GG_NUM_TILE_STATS + GG_CT_DRAM_QUEUE_UTILIZED_NS] = C->t[i].dram_q->util_cycles;
    out[(size_t)i * GG_NUM_TILE_STATS + GG_CT_DRAM_QUEUE_LAST_NS] = C->t[i].dram_q->last_req;
  }
}

void oracle_coh_cache_counters(const oracle_coh* C, uint64_t* out)
{
  for (uint32_t t = 0; t < C->T; ++t) {
    memcpy(out + ((size_t)t * 2 + 0) * GG_NUM_CACHE_COUNTERS, C->t[t].c.l1.c, sizeof(uint64_t) * GG_NUM_CACHE_COUNTERS);
    memcpy(out + ((size_t)t * 2 + 1) * GG_NUM_CACHE_COUNTERS, C->t[t].c.l2.c, sizeof(uint64_t) * GG_NUM_CACHE_COUNTERS);
  }
}

/* The state cache_line_replication.dat is written from (…mosi/memory_manager.cc:
 * 503-551), per tile, by walking the state itself:
 *   lines[t]   = L1-D exclusive, L1-D shared, L2 exclusive, L2 shared lines of
 *                tile t (MODIFIED; OWNED + SHARED, :530-535; no L1-I here);
 *   hist[t][n] = entries of tile t's directory slice with n sharers, the
 *                entries in _replaced_directory_entry_list included: what
 *                Directory::updateSharerStats (directory.cc:55-79) keeps
 *                incrementally for n >= 1 (an entry leaves the list only with
 *                no sharer left).  n is the popcount of the sharer bit vector:
 *                no count kept beside it is read.  Bin 0 (allocated entries
 *                without a sharer) is no part of the reference's output;
 *   pending[t] = entries of the replaced list that still have a sharer.
 * Tiles of other shards stay zero.  Private-L2 protocols only. */
int oracle_coh_census(const oracle_coh* C, uint64_t* lines, uint64_t* hist, uint64_t* pending)
{
  if (C->err) return GG_ERR_STATE;
  if (C->shl2) return GG_ERR_UNSUPPORTED;
  const uint32_t T = C->T, entries = C->dir_sets * C->dir_assoc;
  memset(lines, 0, sizeof(uint64_t) * 4 * T);
  memset(hist, 0, sizeof(uint64_t) * (size_t)T * (T + 1));
  memset(pending, 0, sizeof(uint64_t) * T);
  for (uint32_t t = 0; t < T; ++t) {
    const c_tile* Tl = &C->t[t];
    if (!c_owned(C, t)) continue;
    const o_cache* lv[2] = { &Tl->c.l1, &Tl->c.l2 };
    for (int k = 0; k < 2; ++k)
      for (size_t i = 0; i < (size_t)lv[k]->sets * lv[k]->ways; ++i) {
        const uint32_t cs = lv[k]->lines[i].cstate;
        if (cs == GG_CSTATE_MODIFIED) lines[4 * t + 2 * k]++;
        else if (cs == GG_CSTATE_SHARED || cs == GG_CSTATE_OWNED) lines[4 * t + 2 * k + 1]++;
      }
    uint64_t* h = hist + (size_t)t * (T + 1);
    for (uint32_t i = 0; i < entries; ++i) {
      const c_dentry* e = Tl->slot[i];
      if (!e || e->addr == C_INVALID_ADDR) continue;
      h[de_num(C, e)]++;
    }
    for (uint32_t i = 0; i < Tl->nreplaced; ++i) {
      const uint32_t n = de_num(C, Tl->replaced[i]);
      h[n]++;
      if (n) pending[t]++;
    }
  }
  return 0;
}

void oracle_coh_net_counters(const oracle_coh* C, uint64_t* out) { oracle_noc_counters(C->noc, out); }
void oracle_coh_proto_stats(const oracle_coh* C, uint64_t* out)
{
  for (uint32_t i = 0; i < C->T; ++i)
    memcpy(out + (size_t)i * GG_NUM_PROTO_STATS, C->t[i].ps, sizeof(uint64_t) * GG_NUM_PROTO_STATS);
}
void oracle_coh_run_info(const oracle_coh* C, uint64_t* out) { memcpy(out, C->ri, sizeof(C->ri)); }
void oracle_coh_miss_types(const oracle_coh* C, uint64_t* out)
{
  for (uint32_t t = 0; t < C->T; ++t) {
    memcpy(out + ((size_t)t * 2 + 0) * GG_NUM_MISS_TYPES, C->t[t].c.l1.mt, sizeof(uint64_t) * GG_NUM_MISS_TYPES);
    memcpy(out + ((size_t)t * 2 + 1) * GG_NUM_MISS_TYPES, C->t[t].c.l2.mt, sizeof(uint64_t) * GG_NUM_MISS_TYPES);
  }
}

/* All-core CPU baseline (bench.py): one context per logical shard, the
 * shards' quanta in parallel (OpenMP), the quantum-boundary exchange between
 * the contexts — the multi-rank schedule of DESIGN.md §4, so every output
 * equals oracle_coh_run's.  Outputs as oracle_coh_tile_stats /
 * _cache_counters / _net_counters / _run_info (any may be NULL). */
int oracle_coh_run_parallel(const gg_config* cfg, int threads, const uint64_t* addr, const uint32_t* meta,
                            const uint64_t* tile_offsets, uint64_t* access_out, uint64_t* tile_stats,
                            uint64_t* cache, uint64_t* net, uint64_t* run_info)
{
  const uint32_t K = cfg->num_shards ? cfg->num_shards : 1, T = cfg->num_tiles;
  oracle_coh** Cs = (oracle_coh**)calloc(K, sizeof(void*));
  int rc = 0;
  for (uint32_t k = 0; k < K && !rc; ++k) {
    gg_config c = *cfg;
    c.shard_begin = k; c.shard_end = k + 1;
    Cs[k] = oracle_coh_create(&c);
    rc = oracle_coh_begin(Cs[k], addr, meta, tile_offsets, access_out);
  }
  uint64_t (*st)[5] = (uint64_t(*)[5])calloc(K, sizeof(uint64_t[5]));
  int* rcs = (int*)calloc(K, sizeof(int));
  gg_cmsg** out = (gg_cmsg**)calloc(K, sizeof(void*));
  uint64_t* nout = (uint64_t*)calloc(K, sizeof(uint64_t));
  uint64_t* capout = (uint64_t*)calloc(K, sizeof(uint64_t));
  uint64_t q = 0, quanta = 0, steps = 0;
  while (!rc) {
#pragma omp parallel for num_threads(threads) schedule(dynamic, 1)
    for (uint32_t k = 0; k < K; ++k) rcs[k] = oracle_coh_quantum(Cs[k], q, st[k]);
    uint64_t active = 0, blocked = 0, mn = ~0ull, nb = 0, smax = 0;
    for (uint32_t k = 0; k < K; ++k) {
      if (rcs[k]) rc = rcs[k];
      smax = st[k][0] > smax ? st[k][0] : smax;
      active += st[k][3]; blocked += st[k][4]; if (st[k][2] < mn) mn = st[k][2];
    }
    ++quanta; steps += smax;
    if (rc) break;
    for (uint32_t k = 0; k < K; ++k) {                     /* the exchange */
      const uint64_t n = Cs[k]->nbnd;
      if (n > capout[k]) { capout[k] = n + n / 2 + 16; out[k] = (gg_cmsg*)realloc(out[k], sizeof(gg_cmsg) * capout[k]); }
      nout[k] = oracle_coh_export(Cs[k], out[k], capout[k]);
      nb += nout[k];
    }
    for (uint32_t k = 0; k < K && !rc; ++k)
      for (uint64_t i = 0; i < nout[k] && !rc; ++i) {
        const gg_cmsg* m = &out[k][i];
        const uint32_t d = Cs[k]->shard[m->hop == GG_HOP_NONE ? m->dst : m->hop];
        rc = d < K ? oracle_coh_import(Cs[d], m, 1) : GG_ERR_INVALID;
      }
    if (rc) break;
    if (active == 0 && nb == 0) break;
    if (nb == 0 && blocked == 0) { const uint64_t nq = mn / Cs[0]->quantum_ps; q = nq > q + 1 ? nq : q + 1; }
    else if (nb == 0) { rc = GG_ERR_STATE; break; }
    else q = q + 1;
  }
  if (!rc) {
    const size_t ns = (size_t)T * GG_NUM_TILE_STATS, nc = (size_t)T * 2 * GG_NUM_CACHE_COUNTERS,
                 nn = (size_t)T * GG_NUM_NET_COUNTERS;
    uint64_t* tmp = (uint64_t*)malloc(sizeof(uint64_t) * (ns > nc ? (ns > nn ? ns : nn) : (nc > nn ? nc : nn)));
    if (tile_stats) memset(tile_stats, 0, sizeof(uint64_t) * ns);
    if (cache) memset(cache, 0, sizeof(uint64_t) * nc);
    if (net) memset(net, 0, sizeof(uint64_t) * nn);
    if (run_info) memset(run_info, 0, sizeof(uint64_t) * GG_NUM_RUN_INFO);
    for (uint32_t k = 0; k < K; ++k) {
      if (tile_stats) { oracle_coh_tile_stats(Cs[k], tmp); for (size_t i = 0; i < ns; ++i) tile_stats[i] += tmp[i]; }
      if (cache) { oracle_coh_cache_counters(Cs[k], tmp); for (size_t i = 0; i < nc; ++i) cache[i] += tmp[i]; }
      if (net) { oracle_coh_net_counters(Cs[k], tmp); for (size_t i = 0; i < nn; ++i) net[i] += tmp[i]; }
      if (run_info) {
        for (int i = GG_RI_NET_MSGS; i <= GG_RI_BOUNDARY_MSGS; ++i) run_info[i] += Cs[k]->ri[i];
      }
    }
    if (run_info) { run_info[GG_RI_QUANTA] = quanta; run_info[GG_RI_STEPS] = steps; run_info[GG_RI_FINAL_QUANTUM] = q; }
    free(tmp);
  }
  for (uint32_t k = 0; k < K; ++k) { oracle_coh_destroy(Cs[k]); free(out[k]); }
  free(Cs); free(st); free(rcs); free(out); free(nout); free(capout);
  return rc;
}
