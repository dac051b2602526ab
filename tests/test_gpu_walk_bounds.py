"""The pipelined hop-by-hop walker (k_c_walk<true, RQ>, one wave per router
position) releases a packet by per-packet lower bounds: a candidate still at
an upstream position pp with time tt cannot reach the port before
tt + d * zps.  Every case is one bit-exact comparison against the oracle
(access words, tile statistics, cache and NoC counters) on the smallest shape
that reaches its part of the pipeline loop.

The packet counts in the docstrings are those of the diagnostics build
(GG_COH_DIAG, GG_COH_PROFILE=1: "most packets in one run X .. Y ..", one run
of each case on an MI355X); a run past 64 packets gives a lane a second
candidate, one past 128 takes the one-wave sweep for that launch.  Neither
case a nor case b reaches 64 packets in one run, at 4 hot lines or fewer (a:
39 / 35, 31 / 31, 32 / 53 in X / Y at 3, 2, 1 hot lines; b: 37 / 33, 55 / 31,
27 / 54), so both stay as stated and case i is there for the second
candidate."""
import pytest

from graphite_amd import config as C
from tests.coherent_util import _compare

pytestmark = pytest.mark.gpu

HBH = C.NET_EMESH_HOP_BY_HOP


def _run(T, N, hot, K=1, hot_frac256=51, **kw):
    from oracle import pyoracle as po
    cfg = C.default_config(T, num_shards=K, net_model=HBH, **kw)
    a, m, o = po.gen_trace(T, N, hot_lines=hot, hot_frac256=hot_frac256)
    g = _compare(cfg, a, m, o)
    nc = g[3]
    pk = int(nc[:, C.NET_COUNTERS.index("router_packets")].sum())
    cc = int(nc[:, C.NET_COUNTERS.index("router_contention_cycles")].sum())
    print("router packets %d, contention cycles %d (%.2f per packet), boundary messages %d"
          % (pk, cc, cc / max(pk, 1), int(g[4][C.RUN_INFO.index("boundary_msgs")])))
    if cfg.queue_model_enabled:
        assert cc > 0, "no router contention: no packet was ever delayed at a port"
    if K > 1:
        assert int(g[4][C.RUN_INFO.index("boundary_msgs")]) > 0, "no packet was held at a shard's edge"
    return g


def test_a_runs_of_16_ports_delayed_packets_overtaken():
    """256 tiles x 120, 4 hot lines, one shard: runs of 16 ports, 0.86
    contention cycles per router packet; packets delayed at a port are
    overtaken downstream in key order.  Most packets in one run: X 55, Y 28
    (none past 64)."""
    _run(256, 120, 4)


def test_b_bounds_over_several_ports_zps_5():
    """256 x 100, 4 hot lines, one shard, router 2 + link 3 cycles, 32-bit
    flits: zps of 5 cycles, 5.1 contention cycles per packet; bounds that span
    several ports.  Most packets in one run: X 38, Y 23 (none past 64)."""
    _run(256, 100, 4, router_delay=2, link_delay=3, flit_width=32)


def test_c_shard_edges_off_grid_clock():
    """256 x 100, 2 hot lines, 4 shards at 1.5 GHz: runs cut at shard edges
    with held packets, and the double-precision time conversions in the bound
    and the forward; 0.03 contention cycles per packet.  Most packets in one
    run: X 32, Y 19 (none past 64)."""
    _run(256, 100, 2, K=4, frequency_ghz=1.5)


def test_d_runs_of_8_and_4_ports():
    """256 x 120, 4 hot lines, 8 shards (blocks of 8 x 4 tiles): X runs of 8
    ports, Y runs of 4; 0.07 contention cycles per packet.  Most packets in
    one run: X 48, Y 9 (none past 64)."""
    _run(256, 120, 4, K=8)


def test_e_headline_geometry():
    """1024 x 32, 8 hot lines, 8 shards: the headline's geometry (runs of 16
    and 8 ports), 0.07 contention cycles per packet.  Most packets in one
    run: X 51, Y 18 (none past 64)."""
    _run(1024, 32, 8, K=8)


def test_f_short_runs_first_wave_without_upstream(monkeypatch):
    """16 tiles x 1200, 8 hot lines, 2 shards, per-step launches
    (GG_COH_NO_PERSIST=1): runs of 2-4 ports through the pipeline; the first
    wave has no upstream; 0.09 contention cycles per packet.  Most packets in
    one run: X 11, Y 11 (none past 64)."""
    monkeypatch.setenv("GG_COH_NO_PERSIST", "1")
    _run(16, 1200, 8, K=2)


def test_g_lds_queues_history_list():
    """256 x 100, 4 hot lines, one shard, history_list in the routers and the
    DRAM queue: k_c_walk<true, false>, the ports' queues as LDS images; 0.60
    contention cycles per packet.  Most packets in one run: X 40, Y 27 (none
    past 64)."""
    _run(256, 100, 4, queue_model_type=C.QM_HISTORY_LIST, dram_queue_model_type=C.QM_HISTORY_LIST)


def test_h_no_queue_model():
    """256 x 100, 4 hot lines, one shard, router queue model disabled:
    k_c_walk<true, false> forwarding with pub(0) and no request.  Most
    packets in one run: X 43, Y 27 (none past 64)."""
    _run(256, 100, 4, queue_model_enabled=0)


def test_i_second_candidates_past_64_packets():
    """256 x 120, 16 hot lines taking 255 / 256 of the accesses, one shard: the
    one shape probed that puts more than 64 packets into a pipelined run (two
    launches; most packets in one run: X 72, Y 27), so lanes hold a second
    candidate (packet l + 64) and compare two bound keys; 1.02 contention
    cycles per packet.  The oracle takes 1.9 s on it."""
    _run(256, 120, 16, hot_frac256=255)
