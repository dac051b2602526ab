"""The launch protocol of the device-driven hop-by-hop loop (gg_coherent_run,
per-step launches): a quantum ends in the walker launch of its
last step (quantum_end_walk) instead of a step launch of its own.
GG_COH_QEND_STEP=1 (the step launch ends the quantum, the earlier protocol)
changes which launch does what, never a result: every setting is bit-exact
against the C oracle, run info included.  GG_COH_SPLIT_WALK=1 was the knob of
the fused X + Y walker launch, which was measured and dropped (DESIGN.md §4,
round 8): the build does not read it, and the matrix keeps its two settings
so that a later fused form meets the same cases."""
import functools

import numpy as np
import pytest

from graphite_amd import config as C
from tests.coherent_util import check_invariants
from tests.gpu_util import torch_dev, to_dev, to_np

gpu = pytest.mark.gpu

HBH = C.NET_EMESH_HOP_BY_HOP
SETTINGS = {"default": (), "split_walk": ("GG_COH_SPLIT_WALK",), "qend_step": ("GG_COH_QEND_STEP",),
            "both": ("GG_COH_SPLIT_WALK", "GG_COH_QEND_STEP")}
# (T, N, hot, K, no_persist): more X than Y runs; heavy boundary imports at
# every quantum end; one shard and no boundary records (nsx == nsy); the
# headline's shape in small (nsy > nsx)
SHAPES = [(16, 300, 8, 2, True), (64, 100, 32, 8, True), (256, 150, 64, 1, False), (256, 60, 64, 8, False)]
# what the oracle gives for them (steps, quanta, boundary records), where computed ahead
ORACLE_COUNTS = {(16, 300, 8, 2): (3418, 418, 5683), (64, 100, 32, 8): (2602, 567, 26629),
                 (256, 150, 64, 1): (630, 38, 0), (256, 60, 64, 8): (2185, 407, None)}


def _with_barriers(a, m, offs, every):
    """A BARRIER record after every `every` accesses of each tile (as
    tests/test_gpu_ensemble.py builds its barrier traces)."""
    A, M = [], []
    for t in range(len(offs) - 1):
        s, e = int(offs[t]), int(offs[t + 1])
        pos = np.arange(every, e - s, every)
        A.append(np.insert(a[s:e], pos, np.uint64(0)))
        M.append(np.insert(m[s:e], pos, np.uint32(C.META_BARRIER)))
    o = np.concatenate([[0], np.cumsum([len(x) for x in A])]).astype(np.uint64)
    return np.concatenate(A), np.concatenate(M).astype(np.uint32), o


@functools.lru_cache(maxsize=None)
def _case(T, N, hot, K, barriers=0):
    """The trace and the oracle's run of it, computed once and left unchanged."""
    from oracle import pyoracle as po
    cfg = C.default_config(T, num_shards=K, net_model=HBH)
    r = po.gen_trace(T, N, hot_lines=hot)
    if barriers:
        r = _with_barriers(*r, barriers)
    a, m, o = (np.ascontiguousarray(x) for x in r)
    oc = po.OracleCoherent(cfg)
    ref = (oc.run(a, m, o), oc.tile_stats(), oc.cache_counters(), oc.net_counters(), oc.run_info())
    for x in ref:
        x.setflags(write=False)
    return cfg, (a, m, o), ref


def _gpu_run(cfg, a, m, o, timing=False):
    torch = torch_dev()
    from graphite_amd import backend as B
    be = B.Backend(cfg)
    if timing:
        be.set_timing(True)
    addr, meta = to_dev(torch, a, torch.int64), to_dev(torch, m, torch.int32)
    out = torch.zeros(len(a), dtype=torch.int64, device="cuda")
    be.coherent_run(addr, meta, o, out)
    torch.cuda.synchronize()
    st, cc, ri = be.coherent_stats()
    launches = {k: be.kernel_stats(k)[1] for k in ("coherent_step", "coherent_walk_x", "coherent_walk_y")} if timing else None
    g = (to_np(out, np.uint64), st, cc, be.noc_counters(), ri)
    be.close()
    return g, launches


def _compare(case, timing=False):
    cfg, (a, m, o), r = case
    g, launches = _gpu_run(cfg, a, m, o, timing)
    for name, x, y in zip(("access words", "tile stats", "cache counters", "noc counters"), g[:4], r[:4]):
        if not np.array_equal(x, y):
            d = np.argwhere(np.asarray(x) != np.asarray(y))
            raise AssertionError("%s differ at %d places, first %s: gpu %s oracle %s"
                                 % (name, len(d), d[0], np.asarray(x)[tuple(d[0])], np.asarray(y)[tuple(d[0])]))
    for i, k in enumerate(C.RUN_INFO):
        assert g[4][i] == r[4][i], (k, g[4][i], r[4][i])
    n = np.diff(o.astype(np.int64))
    if (m == C.META_BARRIER).sum() == 0:
        check_invariants(g[1], g[2], g[0], o, per_tile_expected=int(n[0]))
    return r[4], launches


def _setenv(monkeypatch, setting, no_persist):
    for k in ("GG_COH_SPLIT_WALK", "GG_COH_QEND_STEP", "GG_COH_NO_PERSIST"):
        monkeypatch.delenv(k, raising=False)
    for k in SETTINGS[setting]:
        monkeypatch.setenv(k, "1")
    if no_persist:
        monkeypatch.setenv("GG_COH_NO_PERSIST", "1")


@gpu
@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("T,N,hot,K,no_persist", SHAPES)
def test_protocol_matrix(T, N, hot, K, no_persist, setting, monkeypatch):
    """Each shape under the four protocol settings, bit-exact against the oracle."""
    _setenv(monkeypatch, setting, no_persist)
    case = _case(T, N, hot, K)
    ri = case[2][4]
    steps, quanta, bnd = ORACLE_COUNTS[(T, N, hot, K)]
    assert int(ri[C.RUN_INFO.index("steps")]) == steps and int(ri[C.RUN_INFO.index("quanta")]) == quanta
    if bnd is not None:
        assert int(ri[C.RUN_INFO.index("boundary_msgs")]) == bnd
    _compare(case)


@gpu
@pytest.mark.parametrize("setting", ["default", "both"])
def test_barrier_release_through_quantum_end(setting, monkeypatch):
    """BARRIER records: the release time goes from the quantum end (in the
    walker launch, or in the step launch) to the next quantum's step 0."""
    _setenv(monkeypatch, setting, True)
    case = _case(64, 120, 32, 8, barriers=30)
    assert int((case[1][1] == C.META_BARRIER).sum()) == 64 * 3
    _compare(case)


@gpu
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_quantum_end_launches_are_gone(setting, monkeypatch):
    """Launch counts of the (256, 60, 64, 8) run: with the quantum end in the
    walker launch the streamed slots stay below steps + quanta (with batches of
    16, 32, ..., 256, 256, ... that is 2288 against 2800 under
    GG_COH_QEND_STEP=1); the X and the Y walk are one launch each per slot
    under every setting (the fused walker launch was measured and dropped)."""
    _setenv(monkeypatch, setting, False)
    ri, n = _compare(_case(256, 60, 64, 8), timing=True)
    steps, quanta = int(ri[C.RUN_INFO.index("steps")]), int(ri[C.RUN_INFO.index("quanta")])
    assert (steps, quanta) == (2185, 407)
    print("launches (%s): %s, steps + quanta = %d" % (setting, n, steps + quanta))
    if "GG_COH_QEND_STEP" in SETTINGS[setting]:
        assert n["coherent_step"] >= steps + quanta
    else:
        assert steps <= n["coherent_step"] < steps + quanta
    assert n["coherent_walk_x"] == n["coherent_step"]
    assert n["coherent_walk_y"] == n["coherent_step"]
