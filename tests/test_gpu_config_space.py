"""The coherent mode and the NoC batch API away from the 1 GHz square-mesh
defaults: clock frequencies at which Latency::toPicosec / Time::toCycles
(time_types.h:81-109) take their double-precision form, meshes with W != H
and tile counts that are no powers of two (tile-id bits, sharer words with a
partly filled last word, walker launches whose X and Y runs differ), flit
widths other than 64, router / link delays other than 1 / 1, DRAM, cache and
directory latencies off their defaults.  The HIP path against the C oracle on
the same traces, bit-exact everywhere; the picosecond conversion also against
the fixture of the reference's own time_types.h (tests/golden/timeconv.u64)."""
import numpy as np
import pytest

from graphite_amd import config as C
from tests.coherent_util import _compare
from tests.gpu_util import torch_dev, to_dev, to_np

pytestmark = pytest.mark.gpu

HC, HBH = C.NET_EMESH_HOP_COUNTER, C.NET_EMESH_HOP_BY_HOP
NETS = {"HC": HC, "HBH": HBH}
OFF_GRID = (1.5, 2.66, 0.75)        # 1000 / f is no integer: the ceil of the conversions does work


def _run(T=16, N=300, hot=8, compare=_compare, **kw):
    """One GPU-against-oracle comparison plus the conditions that keep the
    case from passing emptily: off-grid latencies at an off-grid clock,
    router contention under hop-by-hop, boundary messages across shards."""
    from oracle import pyoracle as po
    cfg = C.default_config(T, **kw)
    a, m, o = po.gen_trace(T, N, hot_lines=hot)
    g = compare(cfg, a, m, o)
    if cfg.frequency_ghz in OFF_GRID:
        assert ((g[0] >> np.uint64(2)) % np.uint64(1000)).any(), "every latency is a multiple of 1000 ps"
    if cfg.net_model == HBH and T >= 6:
        assert int(g[3][:, C.NET_COUNTERS.index("total_contention_ps")].sum()) > 0
    if cfg.net_model == HBH and cfg.num_shards > 1:
        assert int(g[4][C.RUN_INFO.index("boundary_msgs")]) > 0
    return g


# ---- timing ------------------------------------------------------------------
@pytest.mark.parametrize("net", ["HC", "HBH"])
@pytest.mark.parametrize("f", OFF_GRID)
def test_frequency(f, net):
    _run(frequency_ghz=f, net_model=NETS[net])


def test_cache_and_directory_cycles():
    _run(frequency_ghz=1.5, l1d_data_cycles=3, l1d_tags_cycles=2, l2_data_cycles=11, l2_tags_cycles=5,
         dir_access_cycles=7)


def test_short_quantum_off_grid_clock():
    """100 ns quanta at 1.5 GHz over 4 shards: many quantum boundaries fall at
    times that are no multiples of 1000 ps."""
    g = _run(frequency_ghz=1.5, quantum_ns=100, net_model=HBH, num_shards=4)
    assert int(g[4][C.RUN_INFO.index("quanta")]) > 10


def test_long_quantum():
    _run(quantum_ns=10000)


@pytest.mark.parametrize("bw,lat", [(3.3, 73), (64.0, 1)])
def test_dram_bandwidth_and_latency(bw, lat):
    _run(dram_bandwidth=bw, dram_latency_ns=lat)


def test_dram_queue_model_disabled():
    _run(dram_queue_model_enabled=0)


@pytest.mark.parametrize("T,N,hot,flit,net", [(16, 300, 8, 16, "HC"),     # a 60-bit request: exactly 4 flits of 16
                                              (16, 300, 8, 20, "HBH"),    # exactly 3 flits of 20
                                              (64, 200, 16, 256, "HBH")])
def test_flit_width(T, N, hot, flit, net):
    _run(T, N, hot, flit_width=flit, net_model=NETS[net])


@pytest.mark.parametrize("rd,ld", [(0, 0), (3, 2)])
def test_router_and_link_delay(rd, ld):
    _run(router_delay=rd, link_delay=ld, net_model=HBH)


@pytest.mark.parametrize("qtype,net", [(C.QM_HISTORY_LIST, "HBH"), (C.QM_BASIC, "HC")])
def test_other_queue_models_off_grid_clock(qtype, net):
    """history_list / basic in the DRAM queue and the routers at 1.5 GHz: the
    general step instance and the walkers without register-held queues."""
    _run(frequency_ghz=1.5, net_model=NETS[net], queue_model_type=qtype, dram_queue_model_type=qtype)


@pytest.mark.parametrize("env", ["GG_COH_NO_PERSIST", "GG_COH_NO_LDS_CACHE"])
def test_launch_forms_off_grid_clock(env, monkeypatch):
    """1.5 GHz hop-by-hop in the per-step launches and in the persistent
    launch on the HBM cache arrays."""
    monkeypatch.setenv(env, "1")
    _run(frequency_ghz=1.5, net_model=HBH)


def test_small_caches_off_grid_clock():
    """A geometry that misses the L2: evictions and write-backs at 1.5 GHz."""
    g = _run(N=2000, frequency_ghz=1.5, l1d_size_kb=1, l1d_assoc=2, l2_size_kb=4, l2_assoc=4)
    assert int(g[2][:, 1, C.CACHE_COUNTERS.index("evictions")].sum()) > 0


@pytest.mark.parametrize("entries", [192, 24])
@pytest.mark.parametrize("net", ["HC", "HBH"])
def test_directory_sets_no_power_of_two(entries, net):
    """48 and 6 directory sets of 4 ways: computeSetIndex folds
    floorLog2(sets)-bit fields (directory_cache.cc:64, 332-348), so the first
    32 / 4 sets are used; replacements occur."""
    g = _run(N=600, hot=16, net_model=NETS[net], num_shards=4 if net == "HBH" else 1, l1d_size_kb=2, l2_size_kb=8,
             dir_total_entries=entries, dir_assoc=4)
    assert int(g[1][:, C.TILE_STATS.index("dir_evictions")].sum()) > 0


def test_directory_of_one_set_is_refused():
    """One set folds 0-bit fields: the reference's computeSetIndex never ends."""
    from graphite_amd import backend as B
    from oracle import pyoracle as po
    torch = torch_dev()
    a, m, o = po.gen_trace(16, 50, hot_lines=8)
    cfg = C.default_config(16, dir_total_entries=4, dir_assoc=4)
    be = B.Backend(cfg)
    try:
        with pytest.raises(B.GGError) as ei:                # the run's set-up refuses, not gg_create
            be.coherent_run(to_dev(torch, a, torch.int64), to_dev(torch, m, torch.int32), o, None)
    finally:
        be.close()
    assert ei.value.code == -3 and "two sets" in str(ei.value)
    with pytest.raises(RuntimeError):                       # and so does the oracle
        po.OracleCoherent(cfg).run(a, m, o)


# ---- mesh shapes ---------------------------------------------------------------
#  T     N   hot K(HBH)  other settings
SHAPES = [
    (2, 200, 8, 1, {}),                                        # 1 x 2
    (6, 200, 8, 2, {}),                                        # 2 x 3
    (12, 300, 8, 3, {}),                                       # 3 x 4
    (20, 300, 8, 5, dict(frequency_ghz=0.75)),                 # 4 x 5
    (72, 100, 16, 8, dict(frequency_ghz=2.66, flit_width=32)),  # 8 x 9: the second sharer word holds 8 bits
    (100, 100, 32, 4, {}),                                     # 10 x 10: sharer words of 64 + 36 bits
    (272, 60, 64, 1, {}),                                      # 16 x 17: X runs on the pipeline, Y runs swept
    (272, 60, 64, 4, dict(frequency_ghz=1.5)),
    (306, 60, 64, 1, {}),                                      # 17 x 18: both directions swept
]


@pytest.mark.parametrize("net", ["HC", "HBH"])
@pytest.mark.parametrize("T,N,hot,K,kw", SHAPES, ids=["T%d-K%d" % (s[0], s[3]) for s in SHAPES])
def test_mesh_shape(T, N, hot, K, kw, net):
    # the shard count belongs to the hop-by-hop run
    _run(T, N, hot, net_model=NETS[net], num_shards=K if net == "HBH" else 1, **kw)


@pytest.mark.parametrize("K", [1, 2])
def test_mesh_with_a_hole_hop_counter(K):
    """10 tiles (3 x 4 with a hole): the contiguous-range shard map."""
    _run(10, 200, 8, net_model=HC, num_shards=K)


def test_mesh_with_a_hole_rejected_under_hop_by_hop():
    """The host refuses the run before any launch (hop_by_hop.cc:55-59)."""
    from graphite_amd import backend as B
    from oracle import pyoracle as po
    torch = torch_dev()
    a, m, o = po.gen_trace(10, 50, hot_lines=8)
    with pytest.raises(B.GGError) as ei:
        be = B.Backend(C.default_config(10, net_model=HBH))
        out = torch.zeros(len(a), dtype=torch.int64, device="cuda")
        be.coherent_run(to_dev(torch, a, torch.int64), to_dev(torch, m, torch.int32), o, out)
    assert "full W x H mesh" in str(ei.value)


def _mosi_compare(cfg, a, m, o):
    from tests.test_gpu_mosi import _compare as cmp
    return cmp(cfg, a, m, o)


def _shl2_compare(cfg, a, m, o):
    from tests.test_gpu_shl2 import _compare as cmp
    return cmp(cfg, a, m, o)


PROTOS = {"mosi": (C.PROTO_MOSI, _mosi_compare), "shl2_msi": (C.PROTO_SHL2_MSI, _shl2_compare),
          "shl2_mesi": (C.PROTO_SHL2_MESI, _shl2_compare)}


@pytest.mark.parametrize("proto", sorted(PROTOS))
@pytest.mark.parametrize("T,N,hot,kw", [
    (12, 300, 8, dict(frequency_ghz=1.5, net_model=HC)),
    (72, 100, 16, dict(net_model=HBH, flit_width=32, router_delay=2, link_delay=3)),
], ids=["T12-HC", "T72-HBH"])
def test_other_protocols(proto, T, N, hot, kw):
    """MOSI (its protocol counters included) and the shared-L2 protocols
    (home = line % tiles) on a 3 x 4 and an 8 x 9 mesh, with their own files'
    comparisons."""
    p, cmp = PROTOS[proto]
    _run(T, N, hot, compare=cmp, protocol=p, **kw)


def test_mosi_100_tiles_sharded():
    _run(100, 100, 32, compare=_mosi_compare, protocol=C.PROTO_MOSI, net_model=HBH, num_shards=4, frequency_ghz=1.5)


# ---- gg_noc_route_batch / gg_noc_route_tree ----------------------------------------
NOC = [(16, dict(frequency_ghz=1.5)),
       (12, dict(frequency_ghz=2.66, flit_width=32)),
       (72, dict(router_delay=2, link_delay=3, frequency_ghz=0.75)),
       (20, dict(flit_width=20)),
       (6, dict(frequency_ghz=3.0)),
       (2, dict(frequency_ghz=1.5))]
NOC_IDS = ["T%d" % t for t, _ in NOC]
NOC_N, NOC_SPAN = 4000, 400000


@pytest.mark.parametrize("net", ["HC", "HBH"])
@pytest.mark.parametrize("T,kw", NOC, ids=NOC_IDS)
def test_noc_batch(T, kw, net):
    """gg_noc_route_batch against OracleNoc: arrival, zero-load and
    contention times of every packet and the counters."""
    from tests.test_gpu_noc import packets, run_noc, oracle_noc
    torch = torch_dev()
    cfg = C.default_config(T, net_model=NETS[net], **kw)
    src, dst, bits, t = packets(T, NOC_N, T + NOC_N, NOC_SPAN)
    be, got = run_noc(torch, cfg, src, dst, bits, t)
    on, ref = oracle_noc(cfg, src, dst, bits, t)
    for g, r in zip(got, ref):
        np.testing.assert_array_equal(g, r)
    np.testing.assert_array_equal(be.noc_counters(), on.counters())
    be.close()
    if net == "HBH":
        assert int(ref[2].sum()) > 0


@pytest.mark.parametrize("T,kw", NOC, ids=NOC_IDS)
def test_noc_broadcast_tree(T, kw):
    """gg_noc_route_tree against OracleNoc.route_tree with every 20th packet a
    broadcast."""
    from tests.test_gpu_noc import packets
    from tests.test_noc_broadcast import run_tree, oracle_tree
    torch = torch_dev()
    cfg = C.default_config(T, net_model=HBH, **kw)
    src, dst, bits, t = packets(T, NOC_N, T + NOC_N, NOC_SPAN)
    dst[::20] = C.BROADCAST
    be, got, bgot = run_tree(torch, cfg, src, dst, bits, t)
    on, ref, bref = oracle_tree(cfg, src, dst, bits, t)
    uni = dst != C.BROADCAST
    for g, r in zip(got, ref):
        np.testing.assert_array_equal(g[uni], r[uni])
    for g, r in zip(bgot, bref):
        np.testing.assert_array_equal(g, r)
    np.testing.assert_array_equal(be.noc_counters(), on.counters())
    be.close()
    assert bref[0].shape[0] == NOC_N // 20


# ---- Latency::toPicosec on the device, known answers ----------------------------------
@pytest.mark.parametrize("c,f", [(1, 2.66), (1000003, 1.5), (7, 0.75), (999, 2.66), (7, 1.5), (999, 3.0),
                                 (1000003, 2.66), (1000003, 0.75), (999, 0.75), (1, 1.5), (7, 2.0), (999, 1.0)])
def test_lat_to_ps_known_answers(c, f):
    """The device's lat_to_ps against the reference's Latency(c, f).toPicosec()
    (tests/golden/timeconv.u64): on a 2-tile hop-counter mesh with
    router_delay = c and link_delay = 0 a 1-bit packet from tile 0 to tile 1
    takes toPicosec(c) for its one hop and toPicosec(1) for its one flit.

    time_to_cycles has no window of its own in the ABI: it feeds the router
    queues' request times only, so the differential hop-by-hop cases of this
    file (coherent runs and NoC batches at 0.75, 1.5, 2.66 and 3.0 GHz, with
    contention asserted) are what covers it on the device; the oracle's copy
    is pinned to the same fixture by tests/test_oracle_golden.py."""
    import golden_util as G
    from graphite_amd import backend as B
    torch = torch_dev()
    freqs, cyc, _, lat, _ = G.timeconv()
    fi = freqs.index(f)
    fix = lambda x: int(lat[fi, int(np.flatnonzero(cyc == np.uint64(x))[0])])
    be = B.Backend(C.default_config(2, net_model=HC, router_delay=c, link_delay=0, frequency_ghz=f))
    send = 12345
    dev = [to_dev(torch, np.array([0], np.uint32), torch.int32), to_dev(torch, np.array([1], np.uint32), torch.int32),
           to_dev(torch, np.array([1], np.uint32), torch.int32), to_dev(torch, np.array([send], np.uint64), torch.int64)]
    outs = [torch.zeros(1, dtype=torch.int64, device="cuda") for _ in range(3)]
    be.noc_route_batch(*dev, *outs)
    torch.cuda.synchronize()
    arrival = int(to_np(outs[0], np.uint64)[0])
    be.close()
    assert arrival - send == fix(c) + fix(1)
    if (c, f) == (1000003, 1.5):
        assert arrival - send == 666669334
    if (c, f) == (1, 2.66):
        assert arrival - send == 752
