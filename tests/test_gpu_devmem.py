"""Regrowth and teardown of the backend's device memory (graphite_amd/csrc/
gg_devmem.h) on the GPU: one context takes a small batch, one large enough
that every scratch group grows again (each site's own growth formula is
crossed), and a small one again, bit-exact against the oracle every time; and
contexts that are created, used and closed over and over do not eat device
memory."""
import numpy as np
import pytest

from graphite_amd import config as C
from graphite_amd import backend as B
from oracle import pyoracle as po
from atac_model import AtacModel
from gpu_util import torch_dev, to_dev, to_np
from test_gpu_noc import packets

gpu = pytest.mark.gpu

# 3000 > 200 + 200 / 4 + 1024: the packet arrays allocated for 200 packets are short
SIZES = (200, 3000, 200)


def with_broadcasts(dst, seed):
    d = dst.copy()
    d[np.random.default_rng(seed).random(len(d)) < 0.05] = C.BROADCAST
    return d


def route(torch, be, T, src, dst, bits, t):
    """One batch through gg_noc_route_batch, or gg_noc_route_tree when it holds broadcasts."""
    n, nb = len(src), int((dst == C.BROADCAST).sum())
    dev = [to_dev(torch, src, torch.int32), to_dev(torch, dst, torch.int32), to_dev(torch, bits, torch.int32),
           to_dev(torch, t, torch.int64)]
    o = [torch.zeros(n, dtype=torch.int64, device="cuda") for _ in range(3)]
    bo = [torch.zeros(nb * T, dtype=torch.int64, device="cuda") for _ in range(3)]
    if nb:
        be.noc_route_tree(*dev, *o, *bo, nb)
    else:
        be.noc_route_batch(*dev, *o)
    torch.cuda.synchronize()
    return [to_np(x, np.uint64) for x in o], [to_np(x, np.uint64).reshape(nb, T) for x in bo]


@gpu
@pytest.mark.parametrize("bcast", [False, True], ids=["batch", "tree"])
def test_hop_by_hop_regrows(bcast):
    torch = torch_dev()
    T = 16
    cfg = C.default_config(T, net_model=C.NET_EMESH_HOP_BY_HOP)
    be = B.Backend(cfg)
    for step, n in enumerate(SIZES):
        if step:
            be.reset()
        src, dst, bits, t = packets(T, n, 100 + step, n * 40)
        on = po.OracleNoc(cfg)
        if bcast:
            dst = with_broadcasts(dst, step)
            assert (dst == C.BROADCAST).any()
            (ra, rz, rc), (ba, bz, bc) = on.route_tree(src, dst, bits, t)
            uni = dst != C.BROADCAST
            got, gotb = route(torch, be, T, src, dst, bits, t)
            for g, r in zip(got, (ra, rz, rc)):
                np.testing.assert_array_equal(g[uni], r[uni], err_msg="step %d" % step)
            for g, r in zip(gotb, (ba, bz, bc)):
                np.testing.assert_array_equal(g, r.reshape(g.shape), err_msg="step %d (deliveries)" % step)
        else:
            ref = on.route(src, dst, bits, t)
            got, _ = route(torch, be, T, src, dst, bits, t)
            for g, r in zip(got, ref):
                np.testing.assert_array_equal(g, r, err_msg="step %d" % step)
            assert int(ref[2].sum()) > 0                          # the queues were met
        np.testing.assert_array_equal(be.noc_counters(), on.counters(), err_msg="step %d" % step)
    be.close()


@gpu
@pytest.mark.parametrize("bcast", [False, True], ids=["unicast", "broadcast"])
def test_atac_regrows(bcast):
    torch = torch_dev()
    T = 64
    cfg = C.default_config(T, net_model=C.NET_ATAC)
    be = B.Backend(cfg)                                           # the default ATAC parameters
    for step, n in enumerate(SIZES):
        if step:
            be.reset()
        src, dst, bits, t = packets(T, n, 200 + step, n * 1000)
        if bcast:
            dst = with_broadcasts(dst, step)
            assert (dst == C.BROADCAST).any()
        m = AtacModel(cfg, C.AtacParams())
        ro, rb = m.route(src, dst, bits, t)
        go, gb = route(torch, be, T, src, dst, bits, t)
        for g, r in zip(go, ro):
            np.testing.assert_array_equal(g, r, err_msg="step %d" % step)
        for g, r in zip(gb, rb):
            np.testing.assert_array_equal(g, r, err_msg="step %d (deliveries)" % step)
        np.testing.assert_array_equal(be.noc_counters(), m.counters(), err_msg="step %d" % step)
        np.testing.assert_array_equal(be.noc_atac_counters(), m.atac_counters(), err_msg="step %d" % step)
    be.close()


@gpu
def test_sharded_replay_regrows():
    """replay_kernel=1: the chunk tables ((chunks + 2 (T + 1)) * 2 + 64: 132 after
    the first batch, 338 needed by the second) and the sharded record buffers
    (an eighth to spare) grow between the batches; the cache state carries on."""
    torch = torch_dev()
    T = 8
    cfg = C.default_config(T, replay_kernel=1)
    be = B.Backend(cfg)
    oc = po.OracleCache(cfg)
    first = 0
    for step, n in enumerate((2000, 40000, 2000)):
        gen = [po.gen_uniform(t, first, n, lines_log2=15) for t in range(T)]   # 2 MiB a tile: the 512 KiB L2 evicts
        addr = np.concatenate([g[0] for g in gen])
        meta = np.concatenate([g[1] for g in gen])
        offs = np.arange(T + 1, dtype=np.uint64) * np.uint64(n)
        first += n
        ref, ref_ev = oc.run(addr, meta, offs, want_evicted=True)
        r = torch.zeros(T * n, dtype=torch.int32, device="cuda")
        e = torch.zeros(T * n, dtype=torch.int64, device="cuda")
        be.cache_access_batch(to_dev(torch, addr, torch.int64), to_dev(torch, meta, torch.int32), offs, r, e)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(to_np(r, np.uint32), ref, err_msg="step %d" % step)
        np.testing.assert_array_equal(to_np(e, np.uint64), ref_ev, err_msg="step %d (evicted)" % step)
        np.testing.assert_array_equal(be.cache_counters(), oc.counters(), err_msg="step %d" % step)
    assert (ref & C.RES_L2_EVICT).any()                           # evictions were reported
    be.close()


@gpu
def test_teardown_returns_device_memory():
    """Twenty contexts one after the other, each with a coherent run, a NoC
    batch and a replay behind it: free device memory after the twentieth close
    is not lower than after the second by more than one context's footprint."""
    torch = torch_dev()
    T, CN, NP, NR = 64, 20, 500, 500
    cfg = C.default_config(T, net_model=C.NET_EMESH_HOP_BY_HOP)
    ca, cm, co = po.gen_trace(T, CN, hot_lines=32)
    caddr, cmeta = to_dev(torch, ca, torch.int64), to_dev(torch, cm, torch.int32)
    cout = torch.zeros(T * CN, dtype=torch.int64, device="cuda")
    src, dst, bits, t = packets(T, NP, 5, NP * 40)
    pk = [to_dev(torch, src, torch.int32), to_dev(torch, dst, torch.int32), to_dev(torch, bits, torch.int32),
          to_dev(torch, t, torch.int64)]
    po_ = [torch.zeros(NP, dtype=torch.int64, device="cuda") for _ in range(3)]
    raddr = torch.empty(T * NR, dtype=torch.int64, device="cuda")
    rmeta = torch.empty(T * NR, dtype=torch.int32, device="cuda")
    rres = torch.empty(T * NR, dtype=torch.int32, device="cuda")
    B.gen_uniform_trace(raddr, rmeta, 0, T, NR, lines_log2=13)
    roffs = np.arange(T + 1, dtype=np.uint64) * np.uint64(NR)
    torch.cuda.synchronize()

    def free():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    first_out = None
    footprint = after2 = after20 = None
    for cycle in range(1, 21):
        before = free()
        be = B.Backend(cfg)
        be.coherent_run(caddr, cmeta, co, cout)
        be.reset()
        be.noc_route_batch(*pk, *po_)
        be.cache_access_batch(raddr, rmeta, roffs, rres)
        if cycle == 1:
            footprint = before - free()
            first_out = to_np(cout, np.uint64).copy()
        be.close()
        if cycle == 2:
            after2 = free()
        if cycle == 20:
            after20 = free()
    np.testing.assert_array_equal(to_np(cout, np.uint64), first_out)   # (every context did the same work)
    print("free device memory: after cycle 2 %d B, after cycle 20 %d B; one context %d B" % (after2, after20, footprint))
    assert footprint > 0
    assert after2 - after20 <= footprint
