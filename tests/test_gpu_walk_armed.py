"""The pipelined hop-by-hop walker (k_c_walk<true, true>) arms a waiting port
with its next serve: the wave picks the upstream candidate with the least
bound key, prunes the port's list if it is full, runs the search half of the
request for that packet at its bound time and keeps the predicted word and
the forward word; when the packet's word becomes the predicted one it stores
the forward word at once and updates the queue afterwards.

Every case is one bit-exact comparison against the oracle (access words, tile
statistics, cache and NoC counters, run info) on a shape that takes the armed
search through one of its branches; the conditions asserted are taken from
the GPU's own counters, which equal the oracle's.  The oracle's figures in the
docstrings are those of the CPU oracle on the same shapes."""
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
    tot = {k: int(nc[:, C.NET_COUNTERS.index(k)].sum())
           for k in ("router_packets", "router_contention_cycles", "analytical_requests")}
    tot["boundary_msgs"] = int(g[4][C.RUN_INFO.index("boundary_msgs")])
    tot["steps"] = int(g[4][C.RUN_INFO.index("steps")])
    print(", ".join("%s %d" % kv for kv in tot.items()))
    return tot


def test_1_analytical_branch_and_prune_in_the_armed_search():
    """256 x 100, 4 hot lines, one shard, max_list_size 8: lists of 8
    intervals are full at most requests, so arming prunes, and requests that
    end before the first interval take the M/G/1 branch of the armed search.
    Oracle: 246 k analytical requests, 701 k contention cycles, 2 143 steps."""
    t = _run(256, 100, 4, max_list_size=8)
    assert t["analytical_requests"] > 0, "no request took the analytical branch"
    assert t["router_contention_cycles"] > 0, "no packet was ever delayed at a port"


def test_2_prune_on_nearly_every_request():
    """256 x 60, 4 hot lines, one shard, max_list_size 4: the list is full
    before nearly every request.  Oracle: 233 k analytical requests."""
    t = _run(256, 60, 4, max_list_size=4)
    assert t["analytical_requests"] > 0, "no request took the analytical branch"
    assert t["router_contention_cycles"] > 0, "no packet was ever delayed at a port"


def test_3_bounds_over_several_ports_off_grid_clock_shard_edges():
    """256 x 100, 4 hot lines, 4 shards at 1.5 GHz, router 2 + link 3 cycles,
    32-bit flits: the predicted word (bound time through the double-precision
    conversions) must equal the word the upstream port forwards, over bounds
    that span several ports, with packets held at shard edges.  Oracle: 62 848
    boundary messages, 115 k contention cycles."""
    t = _run(256, 100, 4, K=4, frequency_ghz=1.5, router_delay=2, link_delay=3, flit_width=32)
    assert t["boundary_msgs"] > 0, "no packet was held at a shard's edge"
    assert t["router_contention_cycles"] > 0, "no packet was ever delayed at a port"


def test_4_short_runs_with_small_lists():
    """256 x 100, 4 hot lines, 8 shards (X runs of 8 ports, Y runs of 4),
    max_list_size 8.  Oracle: 115 839 boundary messages, 159 k analytical
    requests."""
    t = _run(256, 100, 4, K=8, max_list_size=8)
    assert t["boundary_msgs"] > 0, "no packet was held at a shard's edge"
    assert t["analytical_requests"] > 0, "no request took the analytical branch"


def test_5_armed_packet_in_the_second_candidate_slot():
    """256 x 120, 16 hot lines taking 255 / 256 of the accesses, one shard,
    max_list_size 16: the one known shape past 64 packets in a pipelined run
    (test_gpu_walk_bounds, case i), so the armed packet can be a lane's second
    candidate (packet l + 64).  Oracle: 1.95 M contention cycles."""
    t = _run(256, 120, 16, hot_frac256=255, max_list_size=16)
    assert t["router_contention_cycles"] > 0, "no packet was ever delayed at a port"
