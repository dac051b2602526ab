"""Adversarial NoC traffic for gg_noc_route_batch / gg_noc_route_tree under
emesh_hop_by_hop, and pure-numpy predicates that say which chain kernel and
which of its branches a batch reaches ("which traffic reaches
which chain kernel").  No GPU and no project library beyond graphite_amd.config.

Every generator returns (src, dst, bits, t) as test_gpu_noc.packets() does,
seeded and deterministic.  The dispatch thresholds are read from the kernel
sources (thresholds()), never retyped: a retuned threshold moves the edge
cases with it, a renamed one fails the CPU test."""
import functools
import math
import os
import re

import numpy as np

from graphite_amd import config as C

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "graphite_amd", "csrc")
THRESHOLD_NAMES = ("kPipePos", "kPipeBatch", "kPipePk", "kSweepPk", "kSweepPos", "kPortPk", "kStageLdsMax", "kQMaxNoc")


# ---- the thresholds, from the sources -----------------------------------------------------------
def _const_expr(text):
    """Value of a C++ integer constant expression of literals, + - * << and parentheses."""
    e = re.sub(r"(?<=\d)(ull|ul|u|ll)\b", "", text.strip(), flags=re.I)
    if not re.fullmatch(r"[0-9xXa-fA-F\s+\-*()<]+", e) or not e:
        raise ValueError("not a plain integer expression: %r" % text)
    return int(eval(e, {"__builtins__": {}}, {}))


def read_constant(name, sources):
    """`constexpr <type> ... name = <expr>[,;]` in one of the sources; KeyError when the name is gone."""
    for s in sources:
        m = re.search(r"constexpr\s+\w+\s+(?:[^;]*?,\s*)?\b%s\s*=\s*([^,;]+)[,;]" % re.escape(name), s)
        if m:
            return _const_expr(m.group(1))
    raise KeyError("threshold %s is no longer defined in gg_noc.hip / gg_noc_stage.h" % name)


def _struct_bytes(name, text):
    """sizeof a struct of uint32_t / uint64_t / double members (gg_dev.h's queue image parts)."""
    m = re.search(r"struct\s+%s\s*\{(.*?)\};" % name, text, re.S)
    if not m:
        raise KeyError("struct %s is no longer defined in gg_dev.h" % name)
    size = {"uint32_t": 4, "uint64_t": 8, "double": 8}
    body = re.sub(r"//[^\n]*", "", m.group(1))
    total = 0
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ty, names = decl.split(None, 1)
        total += size[ty] * len(names.split(","))
    return total


@functools.lru_cache(maxsize=None)
def thresholds(csrc=CSRC):
    """dict of THRESHOLD_NAMES, kFlitBound (the `nf >= (1u << k)` fall-back of the
    sweep and the pipeline) and the queue image parts (HQueue / HNode bytes)."""
    def text(f):
        with open(os.path.join(csrc, f)) as fh:
            return fh.read()
    noc, stage, dev = text("gg_noc.hip"), text("gg_noc_stage.h"), text("gg_dev.h")
    th = {n: read_constant(n, (noc, stage)) for n in THRESHOLD_NAMES}
    bounds = set(re.findall(r"nf\s*>=\s*\(1u\s*<<\s*(\d+)\)", noc))
    if len(bounds) != 1:
        raise KeyError("the flit bound `nf >= (1u << k)` of the sweep and the pipeline: found %s" % sorted(bounds))
    th["kFlitBound"] = 1 << int(bounds.pop())
    th["HQueueBytes"], th["HNodeBytes"] = _struct_bytes("HQueue", dev), _struct_bytes("HNode", dev)
    return th


def qimg_bytes(max_list_size):
    th = thresholds()
    return (th["HQueueBytes"] + max_list_size * th["HNodeBytes"] + 15) & ~15


# ---- the mesh and the model's arithmetic --------------------------------------------------------
def mesh(T):
    w = int(math.floor(math.sqrt(T)))
    h = -(-T // w)
    assert w * h == T, "emesh_hop_by_hop needs a full W x H mesh"
    return w, h


def lat_to_ps(cycles, f):
    return 1000 * cycles if f == 1.0 else int(math.ceil(1000.0 * cycles / f))


def nflits(bits, flit_width):
    bits = np.asarray(bits, np.int64)
    return -(-bits // flit_width)


def two_sizes(T):
    return C.shmem_modeled_bits(T, False), C.shmem_modeled_bits(T, True)


# ---- predicates ---------------------------------------------------------------------------------
def _routed(T, src, dst):
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    return (src < T) & (dst < T) & (src != dst)


def per_source(T, src, dst):
    """Packets per injection port (a stage skips src == dst)."""
    m = _routed(T, src, dst)
    return np.bincount(np.asarray(src, np.int64)[m], minlength=T)


def per_destination(T, src, dst):
    m = _routed(T, src, dst)
    return np.bincount(np.asarray(dst, np.int64)[m], minlength=T)


def xchain_ids(T, src, dst):
    """xchain_of: row * 2 + (1 rightwards, 0 leftwards), -1 without an X part."""
    w, _ = mesh(T)
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    sx, sy, dx = src % w, src // w, dst % w
    return np.where(_routed(T, src, dst) & (dx != sx), sy * 2 + (dx > sx), -1)


def ychain_ids(T, src, dst):
    """ychain_of: destination column * 2 + (1 upwards, 0 downwards), -1 without a Y part."""
    w, _ = mesh(T)
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    sy, dx, dy = src // w, dst % w, dst // w
    return np.where(_routed(T, src, dst) & (dy != sy), dx * 2 + (dy > sy), -1)


def per_xchain(T, src, dst):
    ids = xchain_ids(T, src, dst)
    return np.bincount(ids[ids >= 0], minlength=2 * mesh(T)[1])


def per_ychain(T, src, dst):
    ids = ychain_ids(T, src, dst)
    return np.bincount(ids[ids >= 0], minlength=2 * mesh(T)[0])


def chain_kernel(cfg):
    """The kernel the host launches for the X and the Y stage: 'pipe', 'sweep' or 'hbm' (k_chain)."""
    th = thresholds()
    w, h = mesh(cfg.num_tiles)
    out = []
    for side in (w, h):
        staged = side * qimg_bytes(cfg.max_list_size) <= th["kStageLdsMax"]
        out.append("hbm" if not staged else "pipe" if max(w, h) <= th["kPipePos"] else "sweep")
    return tuple(out)


def chain_paths(cfg, src, dst, bits):
    """For the X and the Y stage, the path of every non-empty chain: {chain id: 'pipe' | 'sweep' |
    'staged' | 'hbm'}, by the rules of the host dispatch, k_chain_pipe's and chain_sweep's fall-backs."""
    th = thresholds()
    T = cfg.num_tiles
    w, h = mesh(T)
    regq = cfg.queue_model_type == C.QM_HISTORY_TREE and cfg.max_list_size <= th["kQMaxNoc"]
    qm_ok = (not cfg.queue_model_enabled) or regq
    giant = nflits(bits, cfg.flit_width) >= th["kFlitBound"]
    res = []
    for stage, ids, npos in ((0, xchain_ids(T, src, dst), w), (1, ychain_ids(T, src, dst), h)):
        kern = chain_kernel(cfg)[stage]
        paths = {}
        for c in np.unique(ids[ids >= 0]):
            n, bad = int((ids == c).sum()), bool(giant[ids == c].any())
            sweep_ok = n <= th["kSweepPk"] and npos <= th["kSweepPos"] and qm_ok and not bad
            pipe_ok = n <= th["kPipePk"] and npos <= th["kPipePos"] and qm_ok and not bad
            if kern == "hbm":
                paths[int(c)] = "hbm"
            elif kern == "pipe" and pipe_ok:
                paths[int(c)] = "pipe"
            else:
                paths[int(c)] = "sweep" if sweep_ok else "staged"
        res.append(paths)
    return res


def _visits(cfg, src, dst, t):
    """With the queue model off: (stage, chain, position, arrival time) of every port a packet asks
    in its X and Y chains; the arrival after `hops` hops is t + hops * lat_to_ps(router + link)."""
    T = cfg.num_tiles
    w, h = mesh(T)
    zps = lat_to_ps(cfg.router_delay + cfg.link_delay, cfg.frequency_ghz)
    src, dst, t = np.asarray(src, np.int64), np.asarray(dst, np.int64), np.asarray(t, np.uint64)
    sx, sy, dx, dy = src % w, src // w, dst % w, dst // w
    xc, yc = xchain_ids(T, src, dst), ychain_ids(T, src, dst)
    xh, yh = np.abs(dx - sx), np.abs(dy - sy)
    rows = []
    for k in range(max(w, h)):
        m = (xc >= 0) & (xh > k)
        rows.append(np.stack([np.zeros(m.sum(), np.int64), xc[m], (sx + np.sign(dx - sx) * k)[m],
                              (t[m] + np.uint64(k * zps)).astype(np.int64)], 1))
        m = (yc >= 0) & (yh > k)
        rows.append(np.stack([np.ones(m.sum(), np.int64), yc[m], (sy + np.sign(dy - sy) * k)[m],
                              (t[m] + ((xh[m] + k) * zps).astype(np.uint64)).astype(np.int64)], 1))
    return np.concatenate(rows)


def max_equal_time_at_position(cfg, src, dst, t):
    """With the queue model off, the largest number of packets that share one (chain, position, time)."""
    assert not cfg.queue_model_enabled
    v = _visits(cfg, src, dst, t)
    if not len(v):
        return 0
    return int(np.unique(v, axis=0, return_counts=True)[1].max())


def max_start_load(T, src, dst, mask=None):
    """The largest number of packets (of `mask`) that enter one X chain at one position: they sit in
    one start pool of the pipeline (all from one source tile, one direction)."""
    w, _ = mesh(T)
    xc = xchain_ids(T, src, dst)
    m = xc >= 0 if mask is None else (xc >= 0) & mask
    key = xc[m] * w + (np.asarray(src, np.int64)[m] % w)
    return int(np.bincount(key).max()) if len(key) else 0


def non_self_fraction(src, dst):
    return float((np.asarray(src) != np.asarray(dst)).mean())


# ---- generators ---------------------------------------------------------------------------------
def _bits(rng, T, n):
    a, b = two_sizes(T)
    return np.where(rng.random(n) < 0.5, a, b).astype(np.uint32)


def uniform(T, n, seed, span_ps, self_frac=0.05):
    """test_gpu_noc.packets(): uniform pairs, two sizes, sorted uniform times with a 7 ps jitter."""
    rng = np.random.default_rng(seed)
    src = rng.integers(0, T, n).astype(np.uint32)
    dst = rng.integers(0, T, n).astype(np.uint32)
    self_m = rng.random(n) < self_frac
    dst[self_m] = src[self_m]
    bits = _bits(rng, T, n)
    t = np.sort(rng.integers(0, span_ps, n)).astype(np.uint64)
    t[rng.random(n) < 0.1] += np.uint64(7)
    return src, dst, bits, t


def one_chain(T, n, seed, span_ps):
    """Exactly n packets, all in the rightward X chain of row 0 (sources in row 0, destinations in
    a column to the right, any row), nothing else in the batch."""
    w, h = mesh(T)
    rng = np.random.default_rng(seed)
    sx = rng.integers(0, w - 1, n)
    dx = sx + 1 + rng.integers(0, w - 1 - sx)
    dy = rng.integers(0, h, n)
    t = np.sort(rng.integers(0, span_ps, n)).astype(np.uint64)
    return sx.astype(np.uint32), (dy * w + dx).astype(np.uint32), _bits(rng, T, n), t


def one_port(T, n, seed, span_ps, tile, sending):
    """Exactly n packets from `tile` (sending) or to `tile`, the other ends uniform over the other tiles."""
    rng = np.random.default_rng(seed)
    other = rng.integers(0, T - 1, n)
    other = (other + (other >= tile)).astype(np.uint32)
    mine = np.full(n, tile, np.uint32)
    t = np.sort(rng.integers(0, span_ps, n)).astype(np.uint64)
    return (mine, other, _bits(rng, T, n), t) if sending else (other, mine, _bits(rng, T, n), t)


def port_edge(T, n, seed, span_ps):
    """Tile 1 sends exactly n packets and tile T - 2 receives exactly n, in one batch, interleaved in time."""
    a = one_port(T, n, seed, span_ps, 1, True)
    a[1][a[1] == T - 2] = 0                            # keep the receiver's count exact
    b = one_port(T, n, seed + 1, span_ps, T - 2, False)
    b[0][b[0] == 1] = 0                                # and the sender's
    cat = [np.concatenate(x) for x in zip(a, b)]
    order = np.argsort(cat[3], kind="stable")
    return tuple(x[order] for x in cat)


def hotspot_dst(T, n, seed, span_ps, tile=0):
    rng = np.random.default_rng(seed)
    src = rng.integers(0, T, n).astype(np.uint32)
    t = np.sort(rng.integers(0, span_ps, n)).astype(np.uint64)
    return src, np.full(n, tile, np.uint32), _bits(rng, T, n), t


def one_source(T, n, seed, span_ps):
    rng = np.random.default_rng(seed)
    dst = rng.integers(0, T, n).astype(np.uint32)
    t = np.sort(rng.integers(0, span_ps, n)).astype(np.uint64)
    return np.full(n, T - 1, np.uint32), dst, _bits(rng, T, n), t


def synchronized(T, n, seed, at_ps):
    """Uniform pairs, every packet at one time: every tie is broken by the packet index."""
    src, dst, bits, _ = uniform(T, n, seed, 1000, self_frac=0.0)
    return src, dst, bits, np.full(n, at_ps, np.uint64)


def two_bursts(T, n, seed, late_ps=1 << 50):
    """Half of the packets at about 1000 ps, half at about late_ps, each +- 2 ps."""
    src, dst, bits, _ = uniform(T, n, seed, 1000, self_frac=0.0)
    rng = np.random.default_rng(seed + 1)
    t = np.where(np.arange(n) < n // 2, 1000, late_ps).astype(np.int64) + rng.integers(-2, 3, n)
    return src, dst, bits, t.astype(np.uint64)


def shuffled(T, n, seed, span_ps, descending=False):
    """Uniform traffic whose index order and time order are unrelated (or exactly opposite)."""
    src, dst, bits, t = uniform(T, n, seed, span_ps)
    order = np.argsort(t, kind="stable")[::-1] if descending else np.random.default_rng(seed + 7).permutation(n)
    return src[order], dst[order], bits[order], t[order]


def cycle_ties(T, n, seed, span_ps, step_ps=1000):
    """Times are multiples of step_ps in [0, span_ps): many exact ties on cycle boundaries."""
    src, dst, bits, _ = uniform(T, n, seed, 1000)
    rng = np.random.default_rng(seed + 3)
    t = np.sort(rng.integers(0, span_ps // step_ps, n) * step_ps).astype(np.uint64)
    return src, dst, bits, t


def giant_flits(T, n, seed, span_ps, flit_width):
    """Uniform traffic; packets 10 and 11 have kFlitBound - 1 flits, 12 and 13 kFlitBound flits, each with an
    X and a Y part, in four different X chains and four different Y chains."""
    bound = thresholds()["kFlitBound"]
    w, _ = mesh(T)
    src, dst, bits, t = uniform(T, n, seed, span_ps, self_frac=0.0)
    ends = [(0, T - 1), (T - 1, 0), (w, T - 2), (T - 1 - w, 1)]
    for k, (s, d), nf in zip((10, 11, 12, 13), ends, (bound - 1, bound - 1, bound, bound)):
        src[k], dst[k], bits[k] = s, d, nf * flit_width
    return src, dst, bits, t


def with_bad_tiles(T, batch, k_src, k_dst):
    """The batch with packet k_src's source and packet k_dst's destination replaced by tile ids >= T."""
    src, dst, bits, t = (x.copy() for x in batch)
    src[k_src], dst[k_dst] = T, T + 7
    return src, dst, bits, t


def tree_sync(T, n_uni, seed, at_ps):
    """Every tile broadcasts once and n_uni unicasts, all at one time."""
    src, dst, bits, _ = uniform(T, n_uni, seed, 1000, self_frac=0.03)
    rng = np.random.default_rng(seed + 5)
    src = np.concatenate([np.arange(T, dtype=np.uint32), src])
    dst = np.concatenate([np.full(T, C.BROADCAST, np.uint32), dst])
    bits = np.concatenate([_bits(rng, T, T), bits])
    order = rng.permutation(len(src))
    return src[order], dst[order], bits[order], np.full(len(src), at_ps, np.uint64)


def tree_hotspot(T, n, seed, span_ps):
    """Unicasts all to tile 0, every 20th packet a broadcast."""
    src, dst, bits, t = hotspot_dst(T, n, seed, span_ps)
    dst[::20] = C.BROADCAST
    return src, dst, bits, t


# ---- the cases ----------------------------------------------------------------------------------
HBH = dict(net_model=C.NET_EMESH_HOP_BY_HOP)


def _case(T, batch, reaches, tree=False, **cfg_kw):
    kw = dict(HBH)
    kw.update(cfg_kw)
    return dict(T=T, cfg_kw=kw, batch=batch, reaches=reaches, tree=tree)


def _cases():
    th = thresholds()
    sw, pp, pt = th["kSweepPk"], th["kPipePk"], th["kPortPk"]
    c = {}
    c["side33"] = lambda: _case(1089, uniform(1089, 6000, 1, 300_000_000), "sweep")
    # the same mesh with the batch inside 3 us: most packets queue somewhere
    c["side33_dense"] = lambda: _case(1089, uniform(1089, 6000, 1, 3_000_000), "sweep")
    c["side32x33"] = lambda: _case(1056, uniform(1056, 6000, 2, 300_000_000), "sweep")
    c["side66_1g5"] = lambda: _case(4356, uniform(4356, 8000, 3, 300_000_000), "sweep", frequency_ghz=1.5, flit_width=32)
    c["sweep_edge_at"] = lambda: _case(1089, one_chain(1089, sw, 4, 40_000_000), "sweep_last")
    c["sweep_edge_over"] = lambda: _case(1089, one_chain(1089, sw + 1, 4, 40_000_000), "sweep_over")
    c["hbm_list320"] = lambda: _case(1024, uniform(1024, 6000, 5, 300_000_000), "hbm", max_list_size=320)
    c["hbm_list320_dense"] = lambda: _case(1024, uniform(1024, 6000, 5, 3_000_000), "hbm", max_list_size=320)
    c["hbm_side100"] = lambda: _case(10000, uniform(10000, 8000, 6, 300_000_000), "hbm")
    c["hbm_list400_hlist"] = lambda: _case(1024, uniform(1024, 6000, 7, 300_000_000), "hbm",
                                           queue_model_type=C.QM_HISTORY_LIST, max_list_size=400)
    c["hbm_list400_hlist_dense"] = lambda: _case(1024, uniform(1024, 6000, 7, 3_000_000), "hbm",
                                                 queue_model_type=C.QM_HISTORY_LIST, max_list_size=400)
    c["pipe_edge_at"] = lambda: _case(16, one_chain(16, pp, 8, 40_000_000), "pipe_last")
    c["pipe_edge_over"] = lambda: _case(16, one_chain(16, pp + 1, 8, 40_000_000), "pipe_over")
    c["port_edge_at"] = lambda: _case(16, port_edge(16, pt, 9, 20_000_000), "port_last")
    c["port_edge_over"] = lambda: _case(16, port_edge(16, pt + 1, 9, 20_000_000), "port_over")
    for T in (16, 64, 1024):
        c["hotspot_dst_%d" % T] = lambda T=T: _case(T, hotspot_dst(T, 4000, 10 + T, 20_000_000), "hot_dst")
        c["one_source_%d" % T] = lambda T=T: _case(T, one_source(T, 4000, 11 + T, 20_000_000), "hot_src")
    for T in (16, 1024):
        c["sync_t5000_%d" % T] = lambda T=T: _case(T, synchronized(T, 4000, 12 + T, 5000), "sync")
        # all at 0 ps with the analytical (M/G/1) branch off: with it on, a port whose requests all come at
        # cycle 0 has newest == the sum of the service times, arrival and service rate differ by one ulp, and
        # the reference's delay is ~1.8e16 cycles, whose picoseconds overflow UInt64 (Latency::toPicosec's
        # cast is undefined there): no reference exists (test_noc_traffic.py shows it on the oracle's queue)
        c["sync_t0_%d" % T] = lambda T=T: _case(T, synchronized(T, 4000, 13 + T, 0), "sync", analytical_enabled=0)
    # 8000 packets: at 4000 the fullest (chain, position, time) holds ~210, below kPipeBatch
    c["sync_noqueue"] = lambda: _case(16, synchronized(16, 8000, 14, 5000), "index_bisection", queue_model_enabled=0)
    c["two_bursts"] = lambda: _case(16, two_bursts(16, 20000, 15), "time_bisection")
    c["shuffled_order"] = lambda: _case(64, shuffled(64, 6000, 16, 2_000_000), "unordered")
    c["descending_order"] = lambda: _case(64, shuffled(64, 6000, 16, 2_000_000, descending=True), "descending")
    c["cycle_ties_zero_delay"] = lambda: _case(64, cycle_ties(64, 40000, 17, 400_000_000), "ties",
                                               router_delay=0, link_delay=0)
    c["cycle_ties_default_delay"] = lambda: _case(64, cycle_ties(64, 40000, 17, 400_000_000), "ties")
    c["giant_flits"] = lambda: _case(16, giant_flits(16, 200, 18, 2_000_000_000, 64), "giant")
    c["tree_sync_16"] = lambda: _case(16, tree_sync(16, 200, 19, 5000), "tree_sync", tree=True)
    c["tree_sync_64"] = lambda: _case(64, tree_sync(64, 200, 20, 5000), "tree_sync", tree=True)
    c["tree_hotspot"] = lambda: _case(64, tree_hotspot(64, 3000, 21, 20_000_000), "tree_hotspot", tree=True)
    return c


CASES = _cases()


@functools.lru_cache(maxsize=None)
def case(name):
    """One case of the table, built once: dict(T, cfg_kw, batch, reaches, tree)."""
    return CASES[name]()


def case_config(name):
    k = case(name)
    return C.default_config(k["T"], **k["cfg_kw"])
