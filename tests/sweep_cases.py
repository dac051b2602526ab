"""The pairwise configuration sweep of the coherent mode: the factors and their
levels, the pairs no case may hold, the literal case table and build(case).

Every pair of levels of two different factors that CONSTRAINTS allows occurs
in at least one row of CASES (tests/test_sweep_cases.py checks it, and runs the
oracle over every row); tests/test_gpu_sweep.py runs each row on the GPU
against the oracle and through the row's driver.  The table is data under
review: tools/sweep_pairs.py printed it, nothing regenerates it at import.
Plain Python, importable without a GPU."""
import collections

import numpy as np

from graphite_amd import config as C

HC, MAGIC, HBH = C.NET_EMESH_HOP_COUNTER, C.NET_MAGIC, C.NET_EMESH_HOP_BY_HOP
LRU, RR = C.POLICY_LRU, C.POLICY_ROUND_ROBIN

# factor -> [(label, the default_config keywords the level sets)]; the first
# level is the default.  Labels are unique over all factors.
FACTORS = collections.OrderedDict([
    ("protocol", [("msi", dict(protocol=C.PROTO_MSI)), ("mosi", dict(protocol=C.PROTO_MOSI)),
                  ("shl2msi", dict(protocol=C.PROTO_SHL2_MSI)), ("shl2mesi", dict(protocol=C.PROTO_SHL2_MESI))]),
    ("net", [("hc", dict(net_model=HC)), ("magic", dict(net_model=MAGIC)), ("hbh", dict(net_model=HBH))]),
    # W x H mesh and shards: two mesh dimensions, more than one shard, sharer words past 64 tiles
    ("mesh", [("4x4k4", dict(num_tiles=16, num_shards=4)), ("2x3k2", dict(num_tiles=6, num_shards=2)),
              ("3x4k3", dict(num_tiles=12, num_shards=3)), ("4x5k5", dict(num_tiles=20, num_shards=5)),
              ("8x9k8", dict(num_tiles=72, num_shards=8)), ("4x4k1", dict(num_tiles=16, num_shards=1))]),
    ("router_queue", [("tree", dict(queue_model_type=C.QM_HISTORY_TREE)), ("tree3", dict(max_list_size=3)),
                      ("tree129", dict(max_list_size=129)),         # past the register-held queues (128)
                      ("list", dict(queue_model_type=C.QM_HISTORY_LIST)),
                      ("listni", dict(queue_model_type=C.QM_HISTORY_LIST, history_list_no_interleaving=1)),
                      ("basic", dict(queue_model_type=C.QM_BASIC)), ("rqoff", dict(queue_model_enabled=0))]),
    ("dram_queue", [("dtree", dict(dram_queue_model_type=C.QM_HISTORY_TREE)),
                    ("dlist", dict(dram_queue_model_type=C.QM_HISTORY_LIST)),
                    ("dbasic", dict(dram_queue_model_type=C.QM_BASIC)), ("dqoff", dict(dram_queue_model_enabled=0))]),
    ("clock", [("1g", dict(frequency_ghz=1.0)), ("1g5", dict(frequency_ghz=1.5)), ("2g66", dict(frequency_ghz=2.66)),
               ("0g75", dict(frequency_ghz=0.75))]),
    ("geometry", [("geo", {}), ("small", dict(l1d_size_kb=1, l1d_assoc=2, l2_size_kb=4, l2_assoc=4)),
                  ("l2a16", dict(l2_assoc=16)), ("l1a8", dict(l1d_assoc=8))]),
    ("policy", [("lru", dict(l1d_policy=LRU, l2_policy=LRU)), ("rr1", dict(l1d_policy=RR, l2_policy=LRU)),
                ("rr2", dict(l1d_policy=LRU, l2_policy=RR)), ("rr12", dict(l1d_policy=RR, l2_policy=RR))]),
    ("directory", [("dauto", {}), ("d192", dict(dir_total_entries=192, dir_assoc=4)),
                   ("d24", dict(dir_total_entries=24, dir_assoc=4))]),
    ("flit", [("f64", dict(flit_width=64)), ("f16", dict(flit_width=16)), ("f20", dict(flit_width=20)),
              ("f256", dict(flit_width=256))]),
    ("delay", [("rl11", dict(router_delay=1, link_delay=1)), ("rl00", dict(router_delay=0, link_delay=0)),
               ("rl32", dict(router_delay=3, link_delay=2))]),
    ("quantum", [("q1000", dict(quantum_ns=1000)), ("q100", dict(quantum_ns=100)), ("q10000", dict(quantum_ns=10000))]),
    ("dram", [("dr5", {}), ("dr3", dict(dram_bandwidth=3.3, dram_latency_ns=73)),
              ("dr64", dict(dram_bandwidth=64.0, dram_latency_ns=1))]),
    # (the values of tests/test_gpu_config_space.py::test_cache_and_directory_cycles)
    ("cycles", [("cyc", {}), ("cyc3", dict(l1d_data_cycles=3, l1d_tags_cycles=2, l2_data_cycles=11, l2_tags_cycles=5,
                                           dir_access_cycles=7))]),
    ("miss_types", [("mt0", {}),
                    ("mt1", dict(l1i_track_miss_types=1, l1d_track_miss_types=1, miss_track_lines=1024)),
                    ("mt12", dict(l1i_track_miss_types=1, l1d_track_miss_types=1, l2_track_miss_types=1,
                                  miss_track_lines=1024))]),
    # the kind of trace record; no configuration keyword
    ("trace", [("plain", {}), ("barr", {}), ("multi", {}), ("ragged", {})]),
    # how the run is driven; no configuration keyword
    ("driver", [("lone", {}), ("legs", {}), ("win", {}), ("ens", {}), ("round2", {})]),
])
NAMES = list(FACTORS)
LEVEL = {lab: (f, kw) for f, lv in FACTORS.items() for lab, kw in lv}
assert len(LEVEL) == sum(len(lv) for lv in FACTORS.values()), "a label occurs twice"

# pairs of labels no case may hold: what the product refuses, with the line of the refusal
CONSTRAINTS = [
    ("shl2msi", "mt12"),      # gg_coherent.hip:521 / oracle/gg_coherent.inc:2082: the shared L2 tracks no miss types
    ("shl2mesi", "mt12"),     # (the same line: both shared-L2 protocols)
    ("round2", "4x4k1"),      # gg_round.hip:157: one logical shard does not split over two ranks
    ("round2", "3x4k3"),      # (the same line, K % W: neither do three
    ("round2", "4x5k5"),      #  nor five; graphite_amd/coherent.py:32 shard_range says the same)
    # gg_cache.hip:2028 (from gg_create, gg_capi.hip:207): every context allocates the private replay's
    # state, whose kernels (kKernels, gg_cache.hip:1947-1952) take a round-robin policy with a 4-way L1-D
    # over an 8- or 16-way L2 only
    ("small", "rr1"), ("small", "rr2"), ("small", "rr12"), ("l1a8", "rr1"), ("l1a8", "rr2"), ("l1a8", "rr12"),
    # gg_dev.h:64 (gg_coherent.hip:529): the basic DRAM queue's moving-average window of 64 needs
    # 2 * max_list_size >= 65 queue words, and max_list_size is one setting for routers and DRAM
    ("tree3", "dbasic"),
]

BARRIER_EVERY = 40
RAGGED = lambda n: [0, 7, n, 31]            # per-tile lengths, as test_coherent_ragged_and_empty_tiles
MAX_RECORDS, MAX_RECORDS_72 = 2000, 150

# One row per case: accesses per tile, then one label per factor in FACTORS'
# order.  (A multi-line row's accesses become about 2.5 lines each; a BARRIER
# row gets a record more after every 40.)
#
# The rows with (win, q10000) are the only ones above MAX_RECORDS.  A window
# must hold 2 + quantum / L1-D data time records (gg_coh_window.hip:71-72),
# which with a 10 000 ns quantum is 2502 at best (3 cycles at 0.75 GHz): a
# trace of 2000 records is final at the first hand-over, and the three
# hand-overs the GPU test asserts cannot happen.  The pair stays covered, at
# 0.75 GHz with 3 L1-D data cycles and up to 2 * MAX_RECORDS records.
CASES_TEXT = """
  400  msi      hc    4x4k4 tree    dtree  0g75 geo   lru  dauto f64  rl11 q1000  dr5  cyc  mt0  barr   lone
  600  mosi     magic 2x3k2 tree    dlist  1g   l2a16 rr12 d192  f16  rl00 q100   dr3  cyc3 mt1  plain  legs
  178  mosi     hbh   3x4k3 tree129 dbasic 1g5  geo   rr1  d24   f20  rl32 q10000 dr64 cyc  mt12 multi  ens
  396  shl2msi  magic 4x5k5 tree3   dqoff  2g66 small lru  d24   f256 rl11 q100   dr64 cyc3 mt0  ragged win
  100  shl2mesi hbh   8x9k8 list    dbasic 2g66 l2a16 rr2  dauto f20  rl00 q1000  dr5  cyc3 mt1  ragged round2
   97  msi      hc    8x9k8 listni  dqoff  1g   l1a8  lru  d192  f256 rl32 q10000 dr3  cyc  mt12 barr   round2
  228  shl2msi  hc    4x4k1 basic   dtree  1g5  l2a16 rr1  d192  f64  rl00 q100   dr5  cyc  mt1  multi  win
 1000  shl2mesi magic 4x4k1 rqoff   dlist  0g75 geo   rr2  d24   f64  rl32 q10000 dr3  cyc  mt0  plain  legs
  500  shl2msi  hbh   3x4k3 listni  dlist  1g5  l1a8  lru  dauto f16  rl11 q1000  dr5  cyc3 mt0  plain  legs
  400  msi      magic 4x4k4 basic   dtree  2g66 l2a16 rr12 d24   f16  rl32 q10000 dr64 cyc3 mt12 ragged lone
  214  shl2mesi magic 2x3k2 tree129 dqoff  1g   l2a16 rr1  dauto f256 rl11 q1000  dr5  cyc3 mt0  multi  ens
  487  msi      hbh   3x4k3 rqoff   dbasic 0g75 small lru  d192  f64  rl00 q100   dr64 cyc3 mt1  barr   ens
  300  mosi     hc    4x5k5 list    dtree  1g   small lru  dauto f20  rl32 q1000  dr64 cyc  mt12 plain  legs
  400  msi      hbh   4x4k4 tree3   dqoff  1g5  geo   rr2  d192  f256 rl00 q100   dr3  cyc3 mt1  plain  lone
 1478  shl2msi  magic 4x4k1 list    dbasic 1g   geo   rr12 dauto f20  rl11 q1000  dr3  cyc  mt0  barr   win
  300  msi      hc    4x5k5 tree129 dlist  2g66 geo   rr1  d192  f16  rl11 q10000 dr3  cyc  mt1  ragged ens
  585  mosi     hc    2x3k2 tree3   dlist  0g75 l2a16 rr2  d24   f16  rl11 q1000  dr64 cyc  mt12 barr   round2
   50  shl2mesi magic 8x9k8 listni  dlist  0g75 l1a8  lru  d24   f16  rl00 q100   dr64 cyc3 mt1  multi  win
  400  mosi     hbh   4x4k1 tree    dqoff  2g66 l1a8  lru  d24   f64  rl32 q100   dr5  cyc3 mt12 ragged lone
   35  shl2mesi hc    8x9k8 rqoff   dtree  1g5  geo   rr12 d192  f64  rl11 q1000  dr5  cyc3 mt0  multi  round2
  214  msi      hbh   2x3k2 basic   dlist  1g   small lru  dauto f20  rl00 q10000 dr3  cyc  mt0  multi  lone
  500  mosi     hbh   3x4k3 rqoff   dtree  1g   l2a16 rr2  dauto f256 rl00 q100   dr3  cyc  mt12 plain  win
  142  shl2msi  hc    4x4k4 tree3   dtree  1g   l1a8  lru  dauto f20  rl32 q10000 dr5  cyc  mt1  multi  ens
  292  shl2msi  hbh   4x5k5 tree129 dbasic 0g75 l2a16 rr12 dauto f256 rl00 q100   dr5  cyc  mt0  barr   lone
  500  msi      hc    3x4k3 list    dqoff  0g75 geo   rr1  d192  f20  rl11 q100   dr5  cyc  mt0  ragged legs
  100  mosi     hc    8x9k8 basic   dbasic 2g66 geo   rr1  dauto f256 rl11 q1000  dr5  cyc  mt0  plain  legs
  600  shl2msi  magic 2x3k2 list    dbasic 1g5  l1a8  lru  d24   f64  rl32 q100   dr5  cyc  mt0  ragged round2
  390  shl2mesi hc    4x4k4 tree    dbasic 1g5  small lru  dauto f16  rl11 q10000 dr5  cyc  mt0  barr   round2
  107  shl2msi  hc    4x5k5 tree    dtree  1g   geo   rr2  d24   f64  rl11 q1000  dr64 cyc  mt0  multi  ens
  585  shl2mesi hc    2x3k2 listni  dtree  2g66 geo   rr1  dauto f64  rl11 q1000  dr5  cyc  mt0  barr   lone
 1515  msi      hc    4x4k1 tree129 dtree  1g   small lru  dauto f64  rl32 q1000  dr64 cyc  mt0  plain  win
  142  mosi     hc    4x4k4 list    dlist  2g66 geo   rr1  dauto f256 rl11 q10000 dr5  cyc  mt0  multi  legs
  400  mosi     hc    4x4k1 listni  dbasic 1g   l2a16 rr12 dauto f20  rl11 q1000  dr5  cyc  mt0  ragged ens
  500  shl2mesi magic 3x4k3 rqoff   dqoff  2g66 geo   rr12 dauto f16  rl11 q1000  dr5  cyc  mt0  plain  lone
  292  shl2mesi hc    4x5k5 basic   dqoff  1g5  l1a8  lru  dauto f64  rl11 q1000  dr5  cyc  mt0  barr   legs
 1376  shl2msi  hc    2x3k2 rqoff   dtree  1g   l1a8  lru  dauto f20  rl11 q1000  dr5  cyc3 mt0  ragged win
  100  shl2msi  hc    8x9k8 tree    dtree  1g   small lru  dauto f20  rl11 q1000  dr5  cyc  mt0  plain  ens
  100  shl2mesi hc    8x9k8 tree3   dtree  1g   geo   rr1  dauto f64  rl11 q1000  dr5  cyc  mt0  plain  round2
 3765  msi      hc    4x4k1 tree    dtree  0g75 geo   rr1  dauto f256 rl11 q10000 dr5  cyc3 mt0  plain  win
  500  msi      hc    3x4k3 basic   dtree  0g75 geo   rr2  dauto f64  rl11 q1000  dr5  cyc  mt0  plain  ens
  100  msi      hc    8x9k8 list    dtree  1g   l2a16 lru  dauto f16  rl11 q1000  dr5  cyc  mt0  plain  lone
  400  msi      hc    4x4k1 tree3   dtree  1g   geo   rr12 dauto f16  rl11 q1000  dr5  cyc  mt0  plain  legs
  400  msi      hc    4x4k4 tree129 dtree  1g   geo   rr2  dauto f64  rl11 q1000  dr5  cyc  mt0  plain  legs
  100  msi      hc    8x9k8 tree129 dtree  1g   l1a8  lru  dauto f64  rl11 q1000  dr5  cyc  mt0  plain  round2
 1376  msi      hc    4x4k4 listni  dtree  1g   small lru  dauto f64  rl11 q1000  dr5  cyc3 mt0  plain  win
  400  msi      hc    4x4k4 rqoff   dtree  1g   geo   rr1  dauto f64  rl11 q1000  dr5  cyc  mt0  plain  lone
  300  msi      hc    4x5k5 listni  dtree  1g   geo   rr2  dauto f64  rl11 q1000  dr5  cyc  mt0  plain  lone
  500  msi      hc    3x4k3 tree    dtree  1g   geo   lru  dauto f64  rl11 q1000  dr5  cyc  mt0  plain  lone
  500  msi      hc    3x4k3 tree3   dtree  1g   geo   lru  dauto f64  rl11 q1000  dr5  cyc  mt0  plain  lone
  300  msi      hc    4x5k5 rqoff   dtree  1g   geo   lru  dauto f64  rl11 q1000  dr5  cyc  mt0  plain  lone
  400  msi      hc    4x4k4 basic   dtree  1g   geo   lru  dauto f64  rl11 q1000  dr5  cyc  mt0  plain  round2
  400  msi      hc    4x4k4 list    dtree  1g   geo   lru  dauto f64  rl11 q1000  dr5  cyc  mt0  plain  ens
"""

Case = collections.namedtuple("Case", "index n labels id")


def _parse(text):
    out = []
    for line in text.strip().splitlines():
        w = line.split()
        if not w or w[0].startswith("#"):
            continue
        labels = tuple(w[1:])
        assert len(labels) == len(NAMES) and all(LEVEL[l][0] == f for l, f in zip(labels, NAMES)), line
        out.append(Case(len(out), int(w[0]), labels, "%02d-%s" % (len(out), "-".join(labels))))
    return out


CASES = _parse(CASES_TEXT)


def level(case, factor):
    return case.labels[NAMES.index(factor)]


def config_kw(case):
    """The default_config keywords of a case (num_tiles among them)."""
    kw = {}
    for lab in case.labels:
        kw.update(LEVEL[lab][1])
    return kw


def config(case, **over):
    kw = config_kw(case)
    kw.update(over)
    return C.default_config(kw.pop("num_tiles"), **kw)


def hot_lines(case):
    return 16 if config_kw(case)["num_tiles"] >= 64 else 8


def trace(case, n=None, hot=None):
    """(addr, meta, offsets) of the case's kind of trace with n accesses per
    tile over `hot` hot lines (default: the case's own)."""
    from oracle import pyoracle as po
    T = config_kw(case)["num_tiles"]
    n = case.n if n is None else n
    hot = hot_lines(case) if hot is None else hot
    kind = level(case, "trace")
    if kind == "plain":
        return po.gen_trace(T, n, hot_lines=hot)
    if kind == "barr":
        from tests.test_gpu_checkpoint import _with_barriers
        return _with_barriers(*po.gen_trace(T, n, hot_lines=hot), BARRIER_EVERY)
    if kind == "multi":
        from tests.access_util import gen_multiline, split_reference
        la, lm, first, lo = split_reference(*gen_multiline(T, n, hot_lines=hot))
        return la, lm, np.asarray(lo, np.uint64)
    assert kind == "ragged"
    parts = [po.gen_hotspot(t, 0, RAGGED(n)[t % 4], hot_lines=hot) for t in range(T)]
    o = np.zeros(T + 1, np.uint64)
    o[1:] = np.cumsum([len(p[0]) for p in parts])
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), o


def build(case):
    """(cfg, addr, meta, offsets) of a case, on the CPU."""
    return (config(case),) + tuple(trace(case))


def allowed(a, b):
    return (a, b) not in CONSTRAINTS and (b, a) not in CONSTRAINTS


def all_pairs():
    """Every pair of labels of two different factors that CONSTRAINTS allows."""
    labs = [(f, lab) for f in NAMES for lab, _ in FACTORS[f]]
    return {(a, b) for i, (fa, a) in enumerate(labs) for fb, b in labs[i + 1:] if fa != fb and allowed(a, b)}


def pairs_of(labels):
    return {(a, b) for i, a in enumerate(labels) for b in labels[i + 1:]}
