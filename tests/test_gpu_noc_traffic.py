"""gg_noc_route_batch / gg_noc_route_tree under emesh_hop_by_hop on the
adversarial traffic of tests/noc_traffic.py (bursts, hotspots, ties, meshes
beyond the pipeline, queue images beyond LDS, the limits at their edges),
bit for bit against the oracle: arrival, zero-load and contention of every
packet and the counters (whose read also proves that no device error was
raised).  tests/test_noc_traffic.py shows on the CPU that every case reaches
the branch of gg_noc.hip it is named after."""
import functools

import numpy as np
import pytest

from graphite_amd import config as C
from graphite_amd import backend as B
from oracle import pyoracle as po
import netgen_model as M
import noc_traffic as NT
from gpu_util import torch_dev, to_np
from test_gpu_noc import run_noc, oracle_noc, packets
from test_noc_broadcast import run_tree, oracle_tree
from test_noc_traffic import sync_large_packets, synth_load1, SYNC_LARGE, SYNTH_LOAD1

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def oracle_case(name):
    """The oracle's answer for a case of the table, computed once: (per packet, per broadcast, counters)."""
    k, cfg = NT.case(name), NT.case_config(name)
    if k["tree"]:
        on, ref, bref = oracle_tree(cfg, *k["batch"])
    else:
        (on, ref), bref = oracle_noc(cfg, *k["batch"]), None
    return ref, bref, on.counters()


def check_batch(torch, cfg, batch, ref, ref_counters):
    be, got = run_noc(torch, cfg, *batch)
    for name, g, r in zip(("arrival", "zero-load", "contention"), got, ref):
        np.testing.assert_array_equal(g, r, err_msg=name)
    np.testing.assert_array_equal(be.noc_counters(), ref_counters)
    be.close()


@pytest.mark.parametrize("name", [n for n in NT.CASES if not n.startswith("tree_")])
def test_adversarial_batch_matches_oracle(name):
    torch = torch_dev()
    ref, _, ref_counters = oracle_case(name)
    check_batch(torch, NT.case_config(name), NT.case(name)["batch"], ref, ref_counters)


@pytest.mark.parametrize("name", [n for n in NT.CASES if n.startswith("tree_")])
def test_adversarial_tree_batch_matches_oracle(name):
    torch = torch_dev()
    src, dst, bits, t = NT.case(name)["batch"]
    ref, bref, ref_counters = oracle_case(name)
    be, got, bgot = run_tree(torch, NT.case_config(name), src, dst, bits, t)
    uni = dst != C.BROADCAST
    for g, r in zip(got, ref):
        np.testing.assert_array_equal(g[uni], r[uni])
    for g, r in zip(bgot, bref):
        np.testing.assert_array_equal(g, r)
    np.testing.assert_array_equal(be.noc_counters(), ref_counters)
    assert bref[0].shape[0] > 0 and int(bref[2].sum()) > 0
    be.close()


@pytest.mark.parametrize("which", list(SYNC_LARGE))
def test_sync_large_packets_match_oracle(which):
    """Every chain's packets start at one instant, so the pipeline's slab is 1 ps wide, and they drain
    for up to 49 188 000 ps (8 x 8, 8200-flit packets): the pipeline executes only the steps at which
    a position serves.  Walking every 1 ps step ran into kMaxSteps (GG_ERR_STATE from the counters)."""
    torch = torch_dev()
    cfg, batch = sync_large_packets(which)
    on, ref = oracle_noc(cfg, *batch)
    if which == "8x8":
        assert int(ref[2].max()) == 49_188_000
    check_batch(torch, cfg, batch, ref, on.counters())


@pytest.mark.parametrize("T,pattern", SYNTH_LOAD1)
def test_synth_load1_routes_and_reduces_like_oracle(T, pattern):
    """The generator at load 1.0 (every tile sends every cycle), N = 64: generated on the device, routed
    and reduced (gg_noc_latency_stats against numpy over the oracle's arrays)."""
    from test_gpu_netgen import generate, host, route, numpy_stats
    torch = torch_dev()
    cfg, model_batch = synth_load1(T, pattern)
    dev, _ = generate(torch, pattern, T, 64, 1.0, 8, cfg.frequency_ghz, seed=T)
    src, dst, bits, t = host(dev)
    for g, r in zip((src, dst, bits, t), model_batch):
        np.testing.assert_array_equal(g, r)
    be = B.Backend(cfg)
    o = route(torch, be, dev)
    on = po.OracleNoc(cfg)
    ref = on.route(src, dst, bits, t)
    for g, r in zip(o, ref):
        np.testing.assert_array_equal(to_np(g, np.uint64), r)
    np.testing.assert_array_equal(be.noc_counters(), on.counters())
    np.testing.assert_array_equal(B.noc_latency_stats(*dev, *o), numpy_stats(src, dst, t, *ref))
    assert int(ref[2].sum()) > 0
    be.close()


def test_bad_tile_ids_raise_range_and_leave_the_rest_alone():
    """One src >= T and one dst >= T in a valid batch: k_keys leaves the two out of every stage and raises
    the range error, which the next counter read reports in the NoC's words; the other packets are
    routed as the batch without the two."""
    torch = torch_dev()
    T, n = 64, 3000
    cfg = C.default_config(T, net_model=C.NET_EMESH_HOP_BY_HOP)
    good = packets(T, n, 31, 300000)
    bad = NT.with_bad_tiles(T, good, 700, 2100)
    keep = np.ones(n, bool)
    keep[[700, 2100]] = False
    _, ref = oracle_noc(cfg, *(x[keep] for x in good))
    be, got = run_noc(torch, cfg, *bad)
    for g, r in zip(got, ref):
        np.testing.assert_array_equal(g[keep], r)
    assert int(ref[2].sum()) > 0
    with pytest.raises(B.GGError) as e:
        be.noc_counters()
    assert e.value.code == M.RANGE
    msg = str(e.value)
    assert "NoC" in msg and "tile id" in msg and "trace address" not in msg and "compressed-tag" not in msg
    be.close()
