"""Synthetic network traffic on the GPU: the generator
gg_gen_network_traffic bit for bit against tests/netgen_model.py, its batches
through gg_noc_route_batch against the C oracle (ATAC: tests/atac_model.py),
the reduction gg_noc_latency_stats against numpy over the oracle's arrays, the
one-call driver gg_noc_synthetic_run against the three calls, and gg_replay
--synthetic-network against gg_replay --route of the same packets."""
import functools
import itertools
import os
import subprocess

import numpy as np
import pytest

from graphite_amd import config as C
from graphite_amd import backend as B
from oracle import pyoracle as po
import netgen_model as M
from gpu_util import torch_dev, to_dev, to_np

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPLAY = os.path.join(ROOT, "graphite_amd", "host", "gg_replay")
K = {n: i for i, n in enumerate(C.NET_COUNTERS)}


def generate(torch, pattern, T, N, load, packet_bytes=8, f=1.0, seed=0):
    """gg_gen_network_traffic into fresh device tensors: (src, dst, bits, time, last_cycle)."""
    n = T * N
    dev = [torch.full((n,), -1, dtype=torch.int32, device="cuda") for _ in range(3)]
    dev.append(torch.full((n,), -1, dtype=torch.int64, device="cuda"))
    last = torch.full((T,), -1, dtype=torch.int64, device="cuda")
    B.gen_network_traffic(B.TrafficParams(pattern, packet_bytes, load, N, seed), T, f, *dev, last)
    return dev, last


def host(dev, last=None):
    a = [to_np(dev[0], np.uint32), to_np(dev[1], np.uint32), to_np(dev[2], np.uint32), to_np(dev[3], np.uint64)]
    return a + ([to_np(last, np.uint64)] if last is not None else [])


# ---- 1. the generator against the model -------------------------------------------------------
GEN_CASES = [(p, T) for T in (16, 64) for p in M.PATTERNS] + [(p, 12) for p in ("transpose", "tornado", "nearest_neighbor")]


@pytest.mark.parametrize("pattern,T", GEN_CASES)
def test_generator_matches_model(pattern, T):
    """All four arrays and last_cycle, for every N x load x packet size x
    frequency: a lone packet, a last round partly used and an exact round;
    every lane sending, a mix, rounds in which nobody sends; 667 ps cycles."""
    torch = torch_dev()
    names = ("src", "dst", "length_bits", "time_ps", "last_cycle")
    for N, load, pb, f in itertools.product((1, 63, 64, 65, 100), (1.0, 0.5, 0.03), (8, 64), (1.0, 1.5)):
        seed = 1000 * N + pb
        dev, last = generate(torch, pattern, T, N, load, pb, f, seed)
        ref = M.generate(pattern, T, N, load, pb, f, seed)
        for name, g, r in zip(names, host(dev, last), ref):
            np.testing.assert_array_equal(g, r, err_msg="%s: N %d load %g bytes %d f %g" % (name, N, load, pb, f))
    if T == 16 and pattern == "transpose":
        t15 = host(generate(torch, pattern, T, 65, 1.0, 8, 1.5, 3)[0])[3]
        assert t15.reshape(T, 65)[2].tolist() == [667 * c for c in range(65)]


def test_two_seeds_give_different_batches():
    torch = torch_dev()
    a = host(generate(torch, "uniform_random", 16, 100, 0.5, seed=1)[0])
    b = host(generate(torch, "uniform_random", 16, 100, 0.5, seed=2)[0])
    c = host(generate(torch, "uniform_random", 16, 100, 0.5, seed=1)[0])
    assert not np.array_equal(a[3], b[3])
    for x, y in zip(a, c):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(a[1], b[1])          # the destinations do not depend on the seed


def test_generator_without_last_cycle_and_rejections():
    torch = torch_dev()
    T, N = 16, 10
    dev = [torch.zeros(T * N, dtype=torch.int32, device="cuda") for _ in range(3)]
    dev.append(torch.zeros(T * N, dtype=torch.int64, device="cuda"))
    B.gen_network_traffic(B.TrafficParams("tornado", 8, 0.5, N, 5), T, 1.0, *dev)
    for g, r in zip(host(dev), M.generate("tornado", T, N, 0.5, 8, 1.0, 5)):
        np.testing.assert_array_equal(g, r)
    with pytest.raises(B.GGError) as e:
        B.gen_network_traffic(B.TrafficParams("tornado", 8, 1.5, N, 5), T, 1.0, *dev)
    assert e.value.code == M.INVALID


# ---- 2. routing against the oracle, 3. the reduction -----------------------------------------
NET_MODELS = {
    "hop_counter": dict(net_model=C.NET_EMESH_HOP_COUNTER),
    "hop_by_hop": dict(net_model=C.NET_EMESH_HOP_BY_HOP),
    "hop_by_hop_no_queue": dict(net_model=C.NET_EMESH_HOP_BY_HOP, queue_model_enabled=0),
}
ROUTE_CASES = [(T, p, m) for T in (16, 64) for p in ("uniform_random", "transpose", "tornado") for m in NET_MODELS]


def route(torch, be, dev):
    o = [torch.zeros(dev[0].numel(), dtype=torch.int64, device="cuda") for _ in range(3)]
    be.noc_route_batch(*dev, *o)
    torch.cuda.synchronize()
    return o


def numpy_stats(src, dst, t, arr, zl, ct):
    """The words of gg_noc_latency_stats from host arrays."""
    s = np.zeros(B.NUM_NLS, np.uint64)
    m = src != dst
    lat = (arr - t)[m]
    s[B.NLS_PACKETS], s[B.NLS_SELF_PACKETS] = m.sum(), (~m).sum()
    s[B.NLS_LATENCY_PS], s[B.NLS_ZERO_LOAD_PS], s[B.NLS_CONTENTION_PS] = lat.sum(), zl[m].sum(), ct[m].sum()
    if m.any():
        s[B.NLS_MAX_LATENCY_PS], s[B.NLS_LAST_ARRIVAL_PS] = lat.max(), arr[m].max()
    for x in lat:
        s[B.NLS_HIST + int(x).bit_length()] += np.uint64(1)
    return s


@functools.lru_cache(maxsize=None)
def routed(T, pattern, model):
    """One generated batch (N = 100, load 0.5) routed on a fresh context and
    reduced, with the oracle's answer on the same arrays; computed once."""
    torch = torch_dev()
    cfg = C.default_config(T, **NET_MODELS[model])
    dev, _ = generate(torch, pattern, T, 100, 0.5, 8, cfg.frequency_ghz, seed=T)
    be = B.Backend(cfg)
    o = route(torch, be, dev)
    stats = B.noc_latency_stats(*dev, *o)
    src, dst, bits, t = host(dev)
    on = po.OracleNoc(cfg)
    ref = on.route(src, dst, bits, t)
    r = dict(batch=(src, dst, bits, t), got=[to_np(x, np.uint64) for x in o], ref=ref, counters=be.noc_counters(),
             ref_counters=on.counters(), stats=stats)
    be.close()
    return r


@pytest.mark.parametrize("T,pattern,model", ROUTE_CASES)
def test_generated_batch_routes_like_oracle(T, pattern, model):
    r = routed(T, pattern, model)
    for g, x in zip(r["got"], r["ref"]):
        np.testing.assert_array_equal(g, x)
    np.testing.assert_array_equal(r["counters"], r["ref_counters"])
    if model == "hop_by_hop":
        assert r["ref"][2].any(), "the case is meant to queue somewhere"


@pytest.mark.parametrize("T,pattern,model", ROUTE_CASES)
def test_reduction_equals_numpy_over_oracle(T, pattern, model):
    r = routed(T, pattern, model)
    src, dst, bits, t = r["batch"]
    want = numpy_stats(src, dst, t, *r["ref"])
    np.testing.assert_array_equal(r["stats"], want)
    assert r["stats"][B.NLS_LATENCY_PS] == r["counters"][:, K["total_latency_ps"]].sum()
    assert r["stats"][B.NLS_CONTENTION_PS] == r["counters"][:, K["total_contention_ps"]].sum()
    assert r["stats"][B.NLS_PACKETS] + r["stats"][B.NLS_SELF_PACKETS] == len(src)
    assert r["stats"][B.NLS_HIST:].sum() == r["stats"][B.NLS_PACKETS]


def test_generated_batch_routes_like_atac_model():
    from atac_model import AtacModel
    torch = torch_dev()
    T = 16
    cfg = C.default_config(T, net_model=C.NET_ATAC)
    prm = C.AtacParams(cluster_size=4, num_access_points=4)
    dev, _ = generate(torch, "uniform_random", T, 40, 0.5, 8, cfg.frequency_ghz, seed=9)
    be = B.Backend(cfg)
    be.noc_set_atac(prm)
    o = route(torch, be, dev)
    stats = B.noc_latency_stats(*dev, *o)
    src, dst, bits, t = host(dev)
    m = AtacModel(cfg, prm)
    ref, _ = m.route(src, dst, bits, t)
    for g, x in zip(o, ref):
        np.testing.assert_array_equal(to_np(g, np.uint64), x)
    np.testing.assert_array_equal(be.noc_counters(), m.counters())
    np.testing.assert_array_equal(stats, numpy_stats(src, dst, t, *ref))
    # the one-call driver on an ATAC context
    b2 = B.Backend(cfg)
    b2.noc_set_atac(prm)
    np.testing.assert_array_equal(b2.noc_synthetic_run(B.TrafficParams("uniform_random", 8, 0.5, 40, 9)), stats)
    np.testing.assert_array_equal(b2.noc_counters(), be.noc_counters())
    np.testing.assert_array_equal(b2.noc_atac_counters(), be.noc_atac_counters())


def stats_of(torch, src, dst, t, arr, zl=None, ct=None):
    n = len(src)
    z = np.zeros(n, np.uint64)
    a = [to_dev(torch, np.asarray(src, np.uint32), torch.int32), to_dev(torch, np.asarray(dst, np.uint32), torch.int32),
         to_dev(torch, np.zeros(n, np.uint32), torch.int32), to_dev(torch, np.asarray(t, np.uint64), torch.int64),
         to_dev(torch, np.asarray(arr, np.uint64), torch.int64),
         to_dev(torch, z if zl is None else np.asarray(zl, np.uint64), torch.int64),
         to_dev(torch, z if ct is None else np.asarray(ct, np.uint64), torch.int64)]
    return B.noc_latency_stats(*a)


def test_reduction_edge_cases():
    torch = torch_dev()
    # an all-self batch: no packets, nothing else
    n = 700
    ids = np.arange(n) % 16
    s = stats_of(torch, ids, ids, np.arange(n), np.arange(n) + 5)
    assert s[B.NLS_SELF_PACKETS] == n and s.sum() == n
    # latency 0 lands in bin 0, latency 2^k in bin k + 1 (2^k - 1 in bin k); times near 2^63
    lats = [0] + [1 << k for k in range(64)] + [(1 << k) - 1 for k in range(1, 65)]
    t = np.full(len(lats), 12345, np.uint64)
    with np.errstate(over="ignore"):
        arr = t + np.array(lats, np.uint64)
    s = stats_of(torch, np.zeros(len(lats)), np.ones(len(lats)), t, arr, zl=np.arange(len(lats)), ct=np.full(len(lats), 3))
    want = np.zeros(65, np.uint64)
    for x in lats:
        want[x.bit_length()] += np.uint64(1)
    np.testing.assert_array_equal(s[B.NLS_HIST:], want)
    assert want[0] == 1 and want[1] == 2 and want[64] == 2
    assert s[B.NLS_PACKETS] == len(lats) and s[B.NLS_MAX_LATENCY_PS] == (1 << 64) - 1
    assert s[B.NLS_LATENCY_PS] == sum(lats) % (1 << 64)
    assert s[B.NLS_ZERO_LOAD_PS] == sum(range(len(lats))) and s[B.NLS_CONTENTION_PS] == 3 * len(lats)
    assert s[7] == 0
    # more than one workgroup and a ragged tail: 1024 workgroups x 256 lanes and 77 more
    n = 1024 * 256 + 77
    rng = np.random.default_rng(4)
    src = rng.integers(0, 64, n)
    dst = rng.integers(0, 64, n)
    t = rng.integers(0, 1 << 40, n).astype(np.uint64)
    lat = (rng.integers(0, 1 << 30, n) >> rng.integers(0, 30, n)).astype(np.uint64)
    zl = rng.integers(0, 1 << 20, n).astype(np.uint64)
    ct = lat // np.uint64(3)
    s = stats_of(torch, src, dst, t, t + lat, zl, ct)
    m = src != dst
    assert s[B.NLS_PACKETS] == m.sum() and s[B.NLS_SELF_PACKETS] == n - m.sum()
    assert s[B.NLS_LATENCY_PS] == lat[m].sum() and s[B.NLS_ZERO_LOAD_PS] == zl[m].sum()
    assert s[B.NLS_CONTENTION_PS] == ct[m].sum() and s[B.NLS_MAX_LATENCY_PS] == lat[m].max()
    assert s[B.NLS_LAST_ARRIVAL_PS] == (t + lat)[m].max()
    bl = np.frexp(lat[m].astype(np.float64))[1]        # the bit length (below 2^53), 0 for 0
    np.testing.assert_array_equal(s[B.NLS_HIST:], np.bincount(bl, minlength=65).astype(np.uint64))
    # an empty batch
    assert not stats_of(torch, [], [], [], []).any()


# ---- 4. the driver ---------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["hop_counter", "hop_by_hop"])
def test_driver_equals_three_calls(model):
    torch = torch_dev()
    T, pattern = 64, "uniform_random"
    r = routed(T, pattern, model)
    cfg = C.default_config(T, **NET_MODELS[model])
    p = B.TrafficParams(pattern, 8, 0.5, 100, T)
    be = B.Backend(cfg)
    np.testing.assert_array_equal(be.noc_synthetic_run(p), r["stats"])
    np.testing.assert_array_equal(be.noc_counters(), r["counters"])
    # a second run on the same context continues from its queue state, as two batch calls do
    s2 = be.noc_synthetic_run(p)
    b2 = B.Backend(cfg)
    dev = [to_dev(torch, x, dt) for x, dt in zip(r["batch"], (torch.int32, torch.int32, torch.int32, torch.int64))]
    route(torch, b2, dev)
    o = route(torch, b2, dev)
    np.testing.assert_array_equal(be.noc_counters(), b2.noc_counters())
    np.testing.assert_array_equal(s2, B.noc_latency_stats(*dev, *o))
    if model == "hop_by_hop":
        assert not np.array_equal(s2, r["stats"]), "the second batch meets the first one's queues"
    # a smaller and a larger batch on the same context: the scratch is regrown
    small = be.noc_synthetic_run(B.TrafficParams("transpose", 8, 1.0, 3, 1))
    assert small[B.NLS_PACKETS] + small[B.NLS_SELF_PACKETS] == 3 * T
    big = be.noc_synthetic_run(B.TrafficParams("transpose", 8, 1.0, 300, 1))
    assert big[B.NLS_PACKETS] + big[B.NLS_SELF_PACKETS] == 300 * T
    with pytest.raises(B.GGError) as e:
        be.noc_synthetic_run(B.TrafficParams("transpose", 8, 0.0, 3, 1))
    assert e.value.code == M.INVALID


# ---- 5. the command line ---------------------------------------------------------------------
def test_replay_synthetic_network_prints_route_summary(tmp_path):
    torch_dev()
    if not os.path.exists(REPLAY):
        pytest.fail("gg_replay is not built")
    T, N, load, seed = 16, 50, 0.5, 11
    src, dst, bits, t, _ = M.generate("transpose", T, N, load, 8, 1.0, seed)
    rec = np.zeros((len(src), 6), np.uint32)
    rec[:, 0], rec[:, 1], rec[:, 2] = src, dst, bits
    rec[:, 4:6] = t.view(np.uint32).reshape(-1, 2)
    f = tmp_path / "pk.bin"
    rec.tofile(str(f))
    base = [REPLAY, "--tiles", str(T), "--net", "hop_by_hop"]
    a = subprocess.run(base + ["--route", str(f)], capture_output=True, text=True, check=True, timeout=120).stdout.splitlines()
    b = subprocess.run(base + ["--synthetic-network", "transpose", "--load", str(load), "--packets", str(N), "--seed",
                               str(seed)], capture_output=True, text=True, check=True, timeout=120).stdout.splitlines()
    summary = a[len(src):]                              # after one hop line per packet
    assert len(summary) > T and b[:-1] == summary
    on = po.OracleNoc(C.default_config(T, net_model=C.NET_EMESH_HOP_BY_HOP))
    want = numpy_stats(src, dst, t, *on.route(src, dst, bits, t))
    n = float(want[B.NLS_PACKETS])
    assert b[-1] == ("Synthetic Network: packets %d self %d mean latency (ps) %.3f max latency (ps) %d "
                     "mean contention (ps) %.3f last arrival (ps) %d"
                     % (want[B.NLS_PACKETS], want[B.NLS_SELF_PACKETS], float(want[B.NLS_LATENCY_PS]) / n,
                        want[B.NLS_MAX_LATENCY_PS], float(want[B.NLS_CONTENTION_PS]) / n, want[B.NLS_LAST_ARRIVAL_PS]))
    bad = subprocess.run(base + ["--synthetic-network", "zigzag"], capture_output=True, text=True, timeout=120)
    assert bad.returncode == 1 and "Unrecognized traffic pattern" in bad.stderr
