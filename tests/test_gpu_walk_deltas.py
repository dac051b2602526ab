"""The pipelined walker (k_c_walk<true, true>, graphite_amd/csrc/gg_coh_dev.h)
keeps a port's M/G/1 sums as loop-invariant base values and carries what its
serves add to them as deltas (RegQueue::Delta, gg_dev.h): the served count, the
sum of flits, the sum of their squares, the maximum of t + qd + p and the
number of analytical requests.  store() writes base + delta and the analytical
branch of search() forms base + delta mid-launch ("Round 16").

Every case is a whole hop-by-hop run, bit-exact against the CPU oracle in
access words, tile statistics, cache counters, NoC counters (which hold
port_utilized_cycles, port_last_cycles and analytical_requests: the sums) and
run info.  The conditions asserted are computed from the oracle's side of the
comparison (the GPU's arrays equal them)."""
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
    tot["port_utilized_cycles"] = sum(int(nc[:, C.NET_COUNTERS.index("port%d_utilized_cycles" % p)].sum()) for p in range(5))
    tot["boundary_msgs"] = int(g[4][C.RUN_INFO.index("boundary_msgs")])
    tot["steps"] = int(g[4][C.RUN_INFO.index("steps")])
    print(", ".join("%s %d" % kv for kv in tot.items()))
    return tot, g


def test_analytical_requests_four_shards_lists_of_65():
    """256 x 100, 4 hot lines, 4 shards, max_list_size 65: 19 319 analytical
    requests on the oracle.  Their delays come out of base + delta in the
    middle of a launch."""
    t, _ = _run(256, 100, 4, K=4, max_list_size=65)
    assert t["analytical_requests"] > 0, "no request took the analytical branch"
    assert t["port_utilized_cycles"] > 0


def test_analytical_requests_eight_shards_lists_of_128():
    """256 x 100, 4 hot lines, 8 shards, max_list_size 128: 552 analytical
    requests on the oracle, packets held at shard edges."""
    t, _ = _run(256, 100, 4, K=8, max_list_size=128)
    assert t["analytical_requests"] > 0, "no request took the analytical branch"
    assert t["boundary_msgs"] > 0, "no packet was held at a shard's edge"


def test_two_candidates_per_lane():
    """256 x 120, 16 hot lines taking 255 / 256 of the accesses, one shard,
    max_list_size 128: the one committed shape with more than 64 packets in a
    pipelined run, so lanes watch two candidates and a port serves many packets
    in one launch (its deltas add up over them)."""
    t, _ = _run(256, 120, 16, hot_frac256=255, max_list_size=128)
    assert t["router_contention_cycles"] > 0, "no packet was ever delayed at a port"


def test_many_launches_per_port(monkeypatch):
    """64 x 200, 4 hot lines taking half the accesses, one shard, in the
    per-step launches (GG_COH_NO_PERSIST: left alone, a mesh of 64 tiles runs
    in the persistent launch, whose walker is the one-wave sweep with
    per-request accounting and carries no delta).  Every port's queue is stored
    by one pipelined walker launch and loaded by the next, thousands of times:
    store -> load -> store of base + delta."""
    monkeypatch.setenv("GG_COH_NO_PERSIST", "1")
    t, _ = _run(64, 200, 4, hot_frac256=128)
    assert t["steps"] > 100, "few launches: the queues are hardly ever reloaded"
    assert t["router_contention_cycles"] > 0, "no packet was ever delayed at a port"


@pytest.mark.parametrize("env", [None, "GG_COH_NO_PERSIST"])
def test_off_the_defaults(env, monkeypatch):
    """16 x 300, 8 hot lines at 1.5 GHz (the smallest hop-by-hop case of
    tests/test_gpu_config_space.py): the conversions between cycles and
    picoseconds take their double-precision form beside the scalar deltas.  A
    mesh this small runs in the persistent launch, whose walker is the
    one-wave sweep; GG_COH_NO_PERSIST puts the same shape through the per-step
    launches and so through the pipelined walker."""
    import numpy as np
    if env:
        monkeypatch.setenv(env, "1")
    t, g = _run(16, 300, 8, frequency_ghz=1.5)
    assert ((g[0] >> np.uint64(2)) % np.uint64(1000)).any(), "every latency is a multiple of 1000 ps"
    assert t["router_contention_cycles"] > 0, "no packet was ever delayed at a port"
