"""Test helpers for the coherent mode: the oracle as a `graphite_amd.coherent`
engine (CPU), the invariants every coherent run must satisfy, and the
GPU-against-oracle comparison of one run (_gpu_run / _oracle_run / _compare)."""
import numpy as np

from graphite_amd import config as C
from tests.gpu_util import torch_dev, to_dev, to_np


class OracleEngine:
    """oracle.pyoracle.OracleCoherent behind the engine surface of
    graphite_amd.coherent.run (CPU tensors, for the gloo tests)."""

    def __init__(self, cfg, addr, meta, offs):
        from oracle import pyoracle as po
        self.cfg = cfg
        self.o = po.OracleCoherent(cfg)
        self.out = self.o.begin(addr, meta, offs)

    def quantum(self, q):
        return self.o.quantum(q)

    def export(self):
        import torch
        msgs = self.o.export(1 << 20)
        K = self.cfg.num_shards
        at = np.where(msgs["hop"] == C.HOP_NONE, msgs["dst"], msgs["hop"])
        shard = C.shard_map(self.cfg.num_tiles, K)[at]
        counts = np.bincount(shard, minlength=K)
        return torch.from_numpy(msgs.view(np.uint8).copy()), counts

    def import_(self, buf):
        b = buf.cpu().numpy() if hasattr(buf, "cpu") else np.asarray(buf)
        self.o.import_(np.frombuffer(b.tobytes(), dtype=C.CMSG_DTYPE))


def check_invariants(stats, cache, out, offs, per_tile_expected=None):
    """Size-independent properties of a finished coherent run."""
    T = stats.shape[0]
    S = {n: stats[:, i] for i, n in enumerate(C.TILE_STATS)}
    n = np.diff(np.asarray(offs, np.int64))
    if per_tile_expected is not None:
        assert np.array_equal(S["accesses"].astype(np.int64), n)
    assert np.array_equal(S["l1_hits"] + S["l2_hits"] + S["l2_misses"], S["accesses"])
    lvl = (out & 3).astype(np.int64)
    lat = out >> 2
    for t in range(T):
        seg = slice(int(offs[t]), int(offs[t + 1]))
        assert int(lat[seg].sum()) == int(S["latency_ps"][t])
        assert int((lvl[seg] == 0).sum()) == int(S["l1_hits"][t])
        assert int((lvl[seg] == 2).sum()) == int(S["l2_misses"][t])
    # L1-D accesses = trace records; L2 accesses = L1-D misses; L2 misses = directory requests
    assert np.array_equal(cache[:, 0, C.CACHE_COUNTERS.index("accesses")], S["accesses"])
    assert np.array_equal(cache[:, 1, C.CACHE_COUNTERS.index("accesses")],
                          cache[:, 0, C.CACHE_COUNTERS.index("misses")])
    assert np.array_equal(cache[:, 1, C.CACHE_COUNTERS.index("misses")], S["l2_misses"])
    reqs = S["sent_ex_req"] + S["sent_sh_req"]
    assert np.array_equal(reqs, S["l2_misses"])
    # every request gets one reply (MOSI: an UPGRADE_REP for a lone sharer / owner)
    reps = S["sent_ex_rep"].sum() + S["sent_sh_rep"].sum() + S["sent_upgrade_rep"].sum()
    assert reps == reqs.sum()
    assert S["msgs_sent"].sum() == S["msgs_received"].sum()


def _gpu_run(cfg, a, m, o):
    torch = torch_dev()
    from graphite_amd import backend as B
    be = B.Backend(cfg)
    addr, meta = to_dev(torch, a, torch.int64), to_dev(torch, m, torch.int32)
    out = torch.zeros(len(a), dtype=torch.int64, device="cuda")
    be.coherent_run(addr, meta, o, out)
    torch.cuda.synchronize()
    st, cc, ri = be.coherent_stats()
    return to_np(out, np.uint64), st, cc, be.noc_counters(), ri


def _oracle_run(cfg, a, m, o):
    from oracle import pyoracle as po
    oc = po.OracleCoherent(cfg)
    out = oc.run(a, m, o)
    return out, oc.tile_stats(), oc.cache_counters(), oc.net_counters(), oc.run_info()


def _compare(cfg, a, m, o):
    g = _gpu_run(cfg, a, m, o)
    r = _oracle_run(cfg, a, m, o)
    for name, x, y in zip(("access words", "tile stats", "cache counters", "noc counters"), g[:4], r[:4]):
        if not np.array_equal(x, y):
            d = np.argwhere(np.asarray(x) != np.asarray(y))
            raise AssertionError("%s differ at %d places, first %s: gpu %s oracle %s"
                                 % (name, len(d), d[0], np.asarray(x)[tuple(d[0])], np.asarray(y)[tuple(d[0])]))
    for k in ("steps", "net_msgs", "self_msgs", "boundary_msgs"):
        i = C.RUN_INFO.index(k)
        assert g[4][i] == r[4][i], (k, g[4][i], r[4][i])
    check_invariants(g[1], g[2], g[0], o, per_tile_expected=int(o[1] - o[0]))
    return g
