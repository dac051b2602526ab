"""Pins tests/atac_model.py, the Python restatement of the ATAC network model
that tests/test_gpu_atac.py compares the HIP path against: topology known
answers from the reference's formulas, the ENet part against the frozen C
oracle (an ATAC batch that never leaves the ENet is an emesh_hop_by_hop
batch) and the closed-form zero-load latency of the ONet part.  CPU only."""
import numpy as np
import pytest

from graphite_amd import config as C
from oracle import pyoracle as po
from atac_model import AtacModel, AC, NC
from test_gpu_noc import packets


# ---- topology (network_model_atac.cc:587-745, :835-841) --------------------------------------
def test_topology_16_tiles_clusters_of_4():
    cl, ap, hub, star = C.atac_topology(16, C.AtacParams(cluster_size=4, num_access_points=4))
    assert hub.tolist() == [5, 7, 13, 15]
    assert ap.tolist() == list(range(16))                       # 4 access points: every tile is its own
    assert cl.reshape(4, 4).tolist() == [[0, 0, 1, 1], [0, 0, 1, 1], [2, 2, 3, 3], [2, 2, 3, 3]]
    _, ap1, hub1, _ = C.atac_topology(16, C.AtacParams(cluster_size=4, num_access_points=1))
    assert hub1.tolist() == [5, 7, 13, 15]
    assert ap1.tolist() == [int(hub1[c]) for c in cl]           # 1 access point: the hub tile


def test_topology_64_tiles_clusters_of_8_two_access_points():
    """The odd-log2 branches: 8 clusters as 2 x 4, each 4 wide x 2 high; 2
    sub-clusters side by side."""
    cl, ap, hub, star = C.atac_topology(64, C.AtacParams(cluster_size=8, num_access_points=2))
    m = cl.reshape(8, 8)
    assert (m[0:2, 0:4] == 0).all() and (m[0:2, 4:8] == 1).all() and (m[2:4, 0:4] == 2).all() and (m[6:8, 4:8] == 7).all()
    assert hub[0] == 10
    assert sorted(set(ap[cl == 0].tolist())) == [9, 11]
    members = np.flatnonzero(cl == 0)
    assert members[np.argsort(star[members])].tolist() == [0, 8, 1, 9, 2, 10, 3, 11]
    assert star[9] == 3
    for t in range(64):                                        # the nearest access point is in the tile's cluster
        assert cl[ap[t]] == cl[t]


def test_receive_net_is_senders_cluster_mod_nets():
    cfg = C.default_config(16, net_model=C.NET_ATAC)
    for nets in (1, 2, 3):
        m = AtacModel(cfg, C.AtacParams(num_receive_nets=nets))
        for s in range(16):
            d = (s + 8) % 16
            m.route(np.array([s], np.uint32), np.array([d], np.uint32), np.array([64], np.uint32),
                    np.array([10 ** 6 * (s + 1)], np.uint64))
            assert ("rh", int(m.cluster[d]), int(m.cluster[s]) % nets) in m.queues
        assert all(k[2] < nets for k in m.queues if k[0] == "rh")


@pytest.mark.parametrize("bad,msg", [
    (dict(T=32), "perfect square"), (dict(T=36), "power of two"), (dict(cluster_size=3), "cluster_size"),
    (dict(num_access_points=3), "num_access_points"), (dict(cluster_size=2, num_access_points=4), "num_access_points"),
    (dict(cluster_size=16), "fewer than 2 clusters"), (dict(num_receive_nets=0), "num_receive_nets"),
    (dict(laser_modes=0), "laser_modes")])
def test_topology_rejections(bad, msg):
    T = bad.pop("T", 16)
    with pytest.raises(ValueError, match=msg):
        C.atac_topology(T, C.AtacParams(**bad))


# ---- ENet == emesh_hop_by_hop (the part the frozen C oracle pins) --------------------------
@pytest.mark.parametrize("T,n,span", [(16, 3000, 150000), (64, 6000, 300000)])
@pytest.mark.parametrize("freq", [1.0, 1.5])
@pytest.mark.parametrize("qtype", [C.QM_HISTORY_TREE, C.QM_HISTORY_LIST])
def test_enet_only_equals_hop_by_hop_oracle(T, n, span, freq, qtype):
    W = int(np.sqrt(T))
    enet_delay = 2 if qtype == C.QM_HISTORY_LIST else 1
    cfg = C.default_config(T, net_model=C.NET_ATAC, frequency_ghz=freq, queue_model_type=qtype)
    prm = C.AtacParams(global_routing=C.ATAC_DISTANCE_BASED, unicast_distance_threshold=2 * (W - 1),
                       enet_router_delay=enet_delay)
    src, dst, bits, t = packets(T, n, T + n, span)
    m = AtacModel(cfg, prm)
    got, _ = m.route(src, dst, bits, t)
    ocfg = C.default_config(T, net_model=C.NET_EMESH_HOP_BY_HOP, frequency_ghz=freq, queue_model_type=qtype,
                            router_delay=enet_delay, link_delay=1)
    on = po.OracleNoc(ocfg)
    ref = on.route(src, dst, bits, t)
    for g, r in zip(got, ref):
        np.testing.assert_array_equal(g, r)
    assert int(ref[2].sum()) > 0                                # contention was exercised
    cols = [NC[k] for k in ("packets_sent", "flits_sent", "bits_sent", "packets_received", "flits_received",
                            "bits_received", "total_latency_ps", "total_contention_ps")]
    np.testing.assert_array_equal(m.counters()[:, cols], on.counters()[:, cols])
    # the ENet router class of the ATAC counters is the mesh router's
    oc, ac = on.counters(), m.atac_counters()
    for a, b in (("enet_buffer_writes", "buffer_writes"), ("enet_switch_alloc", "switch_alloc"),
                 ("enet_crossbar_one", "crossbar"), ("enet_contention_cycles", "router_contention_cycles"),
                 ("enet_port_packets", "router_packets"), ("enet_link_flits", "link_traversals")):
        np.testing.assert_array_equal(ac[:, AC[a]], oc[:, NC[b]])
    assert not ac[:, AC["send_hub_buffer_writes"]].any()         # nothing left the ENet


# ---- zero-load latency of the ONet part ---------------------------------------------------------
@pytest.mark.parametrize("T,kw", [
    (16, dict(cluster_size=4, num_access_points=1)),
    (64, dict(cluster_size=8, num_access_points=2, receive_net_type=C.ATAC_BTREE)),
    (64, dict(cluster_size=16, num_access_points=4, num_receive_nets=1, enet_router_delay=2, send_hub_router_delay=0,
              receive_hub_router_delay=3, star_net_router_delay=2)),
])
@pytest.mark.parametrize("freq", [1.0, 2.66])
def test_onet_zero_load_closed_form(T, kw, freq):
    prm = C.AtacParams(**kw)
    cfg = C.default_config(T, net_model=C.NET_ATAC, queue_model_enabled=0, frequency_ghz=freq, flit_width=20)
    m = AtacModel(cfg, prm)
    W = int(np.sqrt(T))
    src, dst, bits, t = packets(T, 800, 7 + T, 10 ** 6)
    (arr, zl, ct), _ = m.route(src, dst, bits, t)
    L = po.lib()
    ps = lambda cyc: int(L.oracle_lat_to_ps(int(cyc), freq))
    checked = 0
    for k in range(len(src)):
        s, d = int(src[k]), int(dst[k])
        if s == d or m.cluster[s] == m.cluster[d]:
            continue
        ap = int(m.ap[s])
        hops = abs(s % W - ap % W) + abs(s // W - ap // W)
        e = prm.enet_router_delay + 1
        net = 1 if prm.receive_net_type == C.ATAC_BTREE else prm.star_net_router_delay + 1
        nf = -(-int(bits[k]) // 20)
        want = ps(0) + hops * ps(e) + ps(e) + ps(prm.send_hub_router_delay + 3) + \
            ps(prm.receive_hub_router_delay + net) + ps(nf)
        assert int(zl[k]) == want and int(ct[k]) == 0 and int(arr[k]) == int(t[k]) + want
        checked += 1
    assert checked > 400


def test_broadcast_delivers_to_every_tile_once():
    T = 64
    cfg = C.default_config(T, net_model=C.NET_ATAC, queue_model_enabled=0)
    for laser in (1, 2, 3):
        m = AtacModel(cfg, C.AtacParams(cluster_size=8, num_access_points=2, laser_modes=laser))
        src = np.array([3, 40], np.uint32)
        dst = np.array([C.BROADCAST, C.BROADCAST], np.uint32)
        _, (barr, bzl, bct) = m.route(src, dst, np.array([64, 584], np.uint32), np.array([1000, 5000], np.uint64))
        assert barr.shape == (2, T) and (barr > 0).all() and not bct.any()
        c = m.counters()
        assert (c[:, NC["packets_received"]] == 2).all()           # every tile, the senders included
        assert c[:, NC["packets_broadcasted"]].sum() == 2 and c[3, NC["flits_broadcasted"]] == 1
        a = m.atac_counters().sum(axis=0)
        flits = 1 + 10
        assert a[AC["optical_broadcast_flits"]] == (flits if laser & 2 else 0)
        assert a[AC["optical_unicast_flits"]] == (0 if laser & 2 else flits * 8)
        assert a[AC["star_net_crossbar_all"]] == flits * 8 and a[AC["receive_net_link_flits"]] == flits * 64
