"""RegQueue (graphite_amd/csrc/gg_dev.h) holds a history-tree queue in one
wave's registers as a ring over its 128 positions: logical interval i sits at
position (hd + i) & 127, a full list prunes its oldest interval by moving hd,
and inserts / erases rotate the positions behind a logical index (DESIGN.md
§4).

A. The ring alone: one stream of 6000 requests through
Backend.queue_delay_batch, the queue in one wave's registers for the whole
stream, against the CPU oracle's AVL restatement request by request, at list
sizes around the slot boundary (63, 64, 65) and the ring's size (127, 128: at
128 the head moves with no spare position).  The conditions asserted are
computed from the oracle.

B. The ring in the walkers and the step kernel's ports, whose queues are
stored and reloaded every launch: whole hop-by-hop coherent runs, bit-exact
against the oracle (access words, tile statistics, cache and NoC counters, run
info).  The oracle's figures in the docstrings (requests to a mesh port other
than SELF / list full before the request / fits whose interval splits in
two) were counted on the CPU oracle for the same shapes."""
import ctypes

import numpy as np
import pytest

from graphite_amd import backend as B
from graphite_amd import config as C
from tests.coherent_util import _compare
from tests.gpu_util import torch_dev

pytestmark = pytest.mark.gpu

HBH = C.NET_EMESH_HOP_BY_HOP
N_REQ = 6000
CAPS = [2, 4, 63, 64, 65, 100, 127, 128]
# requests that must find the list full, by list size
MIN_FULL = {2: 500, 4: 900}


def _stream():
    rng = np.random.default_rng(1)
    t = np.maximum(0, 4 * np.arange(N_REQ) + rng.integers(-400, 401, N_REQ)).astype(np.uint64)
    p = rng.integers(1, 7, N_REQ).astype(np.uint64)
    return t, p


_ORACLE = {}


def _oracle(cap):
    """Delays, list-full-before flags and analytical flags of the stream on the
    CPU oracle (computed once per list size)."""
    if cap not in _ORACLE:
        from oracle import pyoracle as po
        L = po.lib()
        L.oracle_htree_size.restype = ctypes.c_uint32
        L.oracle_htree_size.argtypes = [ctypes.c_void_p]
        L.oracle_htree_analytical_requests.restype = ctypes.c_uint64
        L.oracle_htree_analytical_requests.argtypes = [ctypes.c_void_p]
        t, p = _stream()
        h = po.OracleHistoryTree(1, cap, True)
        d = np.zeros(N_REQ, np.uint64)
        full = np.zeros(N_REQ, bool)
        anl = np.zeros(N_REQ, bool)
        a0 = 0
        for i in range(N_REQ):
            full[i] = L.oracle_htree_size(h.h) >= cap
            d[i] = h.delay(int(t[i]), int(p[i]))
            a1 = int(L.oracle_htree_analytical_requests(h.h))
            anl[i] = a1 != a0
            a0 = a1
        _ORACLE[cap] = (d, full, anl)
    return _ORACLE[cap]


@pytest.mark.parametrize("cap", CAPS)
def test_a_ring_alone_matches_the_oracle_request_by_request(cap):
    """Oracle, by list size 2, 4, 63, 64, 65, 100, 127, 128: list full before
    527, 906, 1 287, 1 286, 1 285, 1 250, 1 223, 1 222 requests; 5 462, 5 055,
    then 3 430 delayed; 5 434, 4 932, then 25 analytical."""
    torch_dev()
    t, p = _stream()
    ref, full, anl = _oracle(cap)
    n_full, n_delayed, n_anl = int(full.sum()), int((ref != 0).sum()), int(anl.sum())
    print("cap %d: full before %d, delayed %d, analytical %d" % (cap, n_full, n_delayed, n_anl))
    assert n_full >= MIN_FULL.get(cap, 1200), "the list is rarely full: the head hardly moves"
    assert 0 < n_delayed < N_REQ, "delays all zero or all non-zero"
    assert n_anl >= 1, "no request took the analytical branch"
    be = B.Backend(C.default_config(16, max_list_size=cap))
    got = be.queue_delay_batch(t, p)
    be.close()
    bad = np.nonzero(got != ref)[0]
    assert bad.size == 0, "request %d of %d (t %d, p %d): delay %d, oracle %d; %d differ" % (
        bad[0], N_REQ, t[bad[0]], p[bad[0]], got[bad[0]], ref[bad[0]], bad.size)


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


def test_b1_one_shard_lists_of_128():
    """256 x 100, 4 hot lines, one shard, max_list_size 128.  Oracle: 748 645
    mesh-port requests, 504 740 with the list full, 630 331 splits."""
    t = _run(256, 100, 4, max_list_size=128)
    assert t["router_contention_cycles"] > 0, "no packet was ever delayed at a port"


def test_b2_eight_shards_lists_of_128():
    """256 x 100, 4 hot lines, 8 shards, max_list_size 128.  Oracle: 742 048
    mesh-port requests, 545 128 with the list full, 667 643 splits, 552
    analytical requests."""
    t = _run(256, 100, 4, K=8, max_list_size=128)
    assert t["router_contention_cycles"] > 0, "no packet was ever delayed at a port"
    assert t["analytical_requests"] > 0, "no request took the analytical branch"
    assert t["boundary_msgs"] > 0, "no packet was held at a shard's edge"


def test_b3_more_than_64_packets_in_a_pipelined_run():
    """256 x 120, 16 hot lines taking 255 / 256 of the accesses, one shard,
    max_list_size 128: the one shape with more than 64 packets in a pipelined
    run.  Oracle: 1 735 211 mesh-port requests, 1 179 808 with the list full,
    1 318 740 splits."""
    t = _run(256, 120, 16, hot_frac256=255, max_list_size=128)
    assert t["router_contention_cycles"] > 0, "no packet was ever delayed at a port"


def test_b4_four_shards_lists_of_65():
    """256 x 100, 4 hot lines, 4 shards, max_list_size 65 (one interval in
    the second slot).  Oracle: 743 504 mesh-port requests, 595 091 with the
    list full, 656 978 splits, 19 319 analytical requests."""
    t = _run(256, 100, 4, K=4, max_list_size=65)
    assert t["router_contention_cycles"] > 0, "no packet was ever delayed at a port"
    assert t["analytical_requests"] > 0, "no request took the analytical branch"
    assert t["boundary_msgs"] > 0, "no packet was held at a shard's edge"


def test_b5_small_mesh_long_trace():
    """64 x 200, 4 hot lines taking half the accesses, one shard,
    max_list_size 128.  Oracle: 236 590 mesh-port requests, 169 656 with the
    list full, 198 596 splits."""
    t = _run(64, 200, 4, hot_frac256=128, max_list_size=128)
    assert t["router_contention_cycles"] > 0, "no packet was ever delayed at a port"
