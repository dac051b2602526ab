"""BARRIER records through the multi-rank round (gg_round_pack / _unpack /
_finish, gg_round_exchange, gg_coherent_run_ranks): W contexts on one GPU,
each owning K/W of the logical shards, with a device-copy transport that moves
the slots and the B.ROUND_WORDS status words as opaque bytes.  The release of
a barrier (SimBarrier::wait, sync_server.cc:133-170: every tile with an
unfinished trace waits, all continue at the latest arrival) is decided on the
device from the gathered words of every rank and applied by step 0 of the next
quantum.  Every run must equal one context running gg_coherent_run and the
oracle, bit for bit, and every rank must decide every round alike.

The traces hold quantum ends at which only some tiles wait (a release there
would be wrong), tiles that finish while others still wait (the barrier's
count shrinks), a tile whose first and one whose last record is a BARRIER; the
one CPU test checks with the oracle that they do."""
import ctypes
import functools
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from graphite_amd import capture as cp
from graphite_amd import config as C
from tests.gpu_util import torch_dev, to_np
from tests.gpu_util import to_dev as _to_dev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBH, HC = C.NET_EMESH_HOP_BY_HOP, C.NET_EMESH_HOP_COUNTER


# ---- the traces -----------------------------------------------------------
def _with_barriers(a, m, offs, every):
    """A BARRIER record after every `every` accesses of each tile."""
    A, M = [], []
    for t in range(len(offs) - 1):
        s, e = int(offs[t]), int(offs[t + 1])
        pos = np.arange(every, e - s, every)
        A.append(np.insert(a[s:e], pos, np.uint64(0)))
        M.append(np.insert(m[s:e], pos, np.uint32(C.META_BARRIER)))
    o = np.concatenate([[0], np.cumsum([len(x) for x in A])]).astype(np.uint64)
    return np.concatenate(A), np.concatenate(M), o


def _ragged(T, N, K, every):
    """The hotspot trace whose shard-0 tiles stop after N / 2 accesses; tile
    1's first and tile 2's last record is a BARRIER."""
    from oracle import pyoracle as po
    a, m, o = po.gen_trace(T, N, hot_lines=16)
    sh = C.shard_map(T, K)
    A, M = [], []
    for t in range(T):
        s, e = int(o[t]), int(o[t + 1])
        if sh[t] == 0:
            e = s + N // 2
        at, mt = a[s:e], m[s:e]
        pos = np.arange(every, e - s, every)
        at, mt = np.insert(at, pos, np.uint64(0)), np.insert(mt, pos, np.uint32(C.META_BARRIER))
        if t == 1:
            at, mt = np.insert(at, 0, np.uint64(0)), np.insert(mt, 0, np.uint32(C.META_BARRIER))
        if t == 2:
            at, mt = np.append(at, np.uint64(0)), np.append(mt, np.uint32(C.META_BARRIER))
        A.append(at); M.append(mt)
    offs = np.concatenate([[0], np.cumsum([len(x) for x in A])]).astype(np.uint64)
    return np.concatenate(A), np.concatenate(M).astype(np.uint32), offs


@functools.lru_cache(maxsize=None)
def _trace(kind):
    from oracle import pyoracle as po
    if kind == "hot":                                   # cases 1, 3, 7
        r = _with_barriers(*po.gen_trace(64, 200, hot_lines=16), 50)
    elif kind == "ragged":                              # case 2
        r = _ragged(64, 200, 8, 50)
    elif kind == "proto":                               # case 4
        r = _with_barriers(*po.gen_trace(64, 120, hot_lines=16), 30)
    elif kind == "wide":                                # case 5
        r = _with_barriers(*po.gen_trace(256, 100, hot_lines=16), 25)
    else:                                               # case 6: the reference's fft.C -p16 -m10
        r = cp.load_fft_trace(cp.REAL_FFT_TRACES[10])[:3]
    r = tuple(np.ascontiguousarray(x) for x in r)
    for x in r:
        x.setflags(write=False)
    return r


def to_dev(torch, a, dtype):
    """A device copy of a shared (read-only) trace array."""
    return _to_dev(torch, np.array(a), dtype)


def _cfg(T, K, net, protocol=C.PROTO_MSI, **kw):
    return C.default_config(T, num_shards=K, net_model=net, protocol=protocol, **kw)


@functools.lru_cache(maxsize=None)
def _oracle(kind, T, K, net, protocol=C.PROTO_MSI):
    """(access words, tile stats, NoC counters) of the oracle, computed once."""
    from oracle import pyoracle as po
    a, m, o = _trace(kind)
    oc = po.OracleCoherent(_cfg(T, K, net, protocol))
    r = (oc.run(a, m, o).copy(), oc.tile_stats().copy(), oc.net_counters().copy())
    for x in r:
        x.setflags(write=False)
    return r


_ONE = {}


def _single(torch, kind, T, K, net, protocol=C.PROTO_MSI):
    """The same of one context running gg_coherent_run, once per trace."""
    key = (kind, T, K, net, protocol)
    if key not in _ONE:
        from graphite_amd import backend as B
        a, m, o = _trace(kind)
        be = B.Backend(_cfg(T, K, net, protocol))
        out = torch.zeros(len(a), dtype=torch.int64, device="cuda")
        be.coherent_run(to_dev(torch, a, torch.int64), to_dev(torch, m, torch.int32), o, out)
        torch.cuda.synchronize()
        _ONE[key] = (to_np(out, np.uint64), be.coherent_stats()[0], be.noc_counters())
        be.close()
    return _ONE[key]


# ---- the round over W contexts, device-copy transport ---------------------
def _hip():
    """The HIP runtime the process already uses (torch and libgraphite_gpu share it)."""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            lib = ctypes.CDLL(line.split()[-1])
            lib.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
            lib.hipMemcpy.restype = ctypes.c_int
            return lib
    raise RuntimeError("libamdhip64 is not loaded")


def _copy(hip, dst, src, nbytes):
    if nbytes:
        assert hip.hipMemcpy(ctypes.c_void_p(dst), ctypes.c_void_p(src), nbytes, 3) == 0   # hipMemcpyDeviceToDevice


def _run_ranks(torch, W, T, K, net, protocol, a, m, o, stats):
    """pack / transport / unpack (/ transport / finish) until the run ends;
    (access words, tile stats, NoC counters) summed over the ranks."""
    from graphite_amd import backend as B
    from graphite_amd import coherent as CO
    hip = _hip()
    addr, meta = to_dev(torch, a, torch.int64), to_dev(torch, m, torch.int32)
    bes, outs = [], []
    for r in range(W):
        k0, k1 = CO.shard_range(r, W, K)
        be = B.Backend(_cfg(T, K, net, protocol, shard_begin=k0, shard_end=k1))
        out = torch.zeros(len(a), dtype=torch.int64, device="cuda")
        bes.append(be); outs.append(out)
    try:
        for be, out in zip(bes, outs):
            be.coherent_begin(addr, meta, o, out)
        rb = B.CMSG_RECORD_BYTES
        q, rounds = 0, 0
        while True:
            assert rounds < 100000, "the run did not end"
            ios = [be.round_pack(W, r, q) for r, be in enumerate(bes)]
            torch.cuda.synchronize()
            for r in range(W):                               # transport 1: fixed slots to the peers, words to everyone
                for p in range(W):
                    if p != r:
                        _copy(hip, ios[p].recv + r * ios[p].stride * rb, ios[r].send + p * ios[r].stride * rb,
                              (ios[r].slot + 1) * rb)
                    _copy(hip, ios[p].words_all + r * B.ROUND_WORDS * 8, ios[r].words_own, B.ROUND_WORDS * 8)
            torch.cuda.synchronize()
            for r, be in enumerate(bes):
                be.round_unpack(ios[r])
            rounds += 1
            states = {io.state for io in ios}
            assert len(states) == 1, states                  # every rank decides alike
            state = states.pop()
            if state == B.ROUND_AGAIN:
                stats["again"] += 1
                continue
            if state == B.ROUND_OVERFLOW:
                stats["overflow"] += 1
                for r in range(W):                           # transport 2: the remainder of each slot
                    for p in range(W):
                        n = ios[r].send_count[p]
                        if p != r and n > ios[r].slot:
                            off = 1 + ios[r].slot
                            _copy(hip, ios[p].recv + (r * ios[p].stride + off) * rb,
                                  ios[r].send + (p * ios[r].stride + off) * rb, (n - ios[r].slot) * rb)
                torch.cuda.synchronize()
                for r, be in enumerate(bes):
                    be.round_finish(ios[r])
            assert len({(io.state, io.next_q, io.done) for io in ios}) == 1
            if ios[0].done:
                break
            q = ios[0].next_q
        torch.cuda.synchronize()
        stats["rounds"] = rounds
        got = sum(to_np(x, np.uint64) for x in outs)
        st = sum(be.coherent_stats()[0] for be in bes)
        nc = sum(be.noc_counters() for be in bes)
    finally:
        for be in bes:
            be.close()
    return got, st, nc


def _check(kind, W, T, K, net, protocol=C.PROTO_MSI):
    """ranks == one context == oracle; returns the summed access words and the round counts."""
    torch = torch_dev()
    a, m, o = _trace(kind)
    stats = {"again": 0, "overflow": 0}
    got = _run_ranks(torch, W, T, K, net, protocol, a, m, o, stats)
    one = _single(torch, kind, T, K, net, protocol)
    ref = _oracle(kind, T, K, net, protocol)
    for name, x, y, z in zip(("access words", "tile stats", "noc counters"), got, one, ref):
        assert np.array_equal(x, y), name + ": ranks != one context"
        assert np.array_equal(x, z), name + ": ranks != oracle"
    bar = m == C.META_BARRIER
    assert np.all((got[0][bar] & np.uint64(3)) == C.LVL_SYNC)
    return got, stats


def _plain_knobs(monkeypatch):
    monkeypatch.setenv("GG_ROUND_SLOT", "1024")
    for k in ("GG_ROUND_BATCH0", "GG_ROUND_FAIL_IMPORT", "GG_ROUND_FAIL_FINISH"):
        monkeypatch.delenv(k, raising=False)


@pytest.mark.gpu
@pytest.mark.parametrize("W", [2, 4, 8])
@pytest.mark.parametrize("net", [HBH, HC])
def test_round_barriers_hotspot(W, net, monkeypatch):
    """Case 1: 64 tiles, a barrier after every 50 of 200 accesses."""
    _plain_knobs(monkeypatch)
    _check("hot", W, 64, 8, net)


@pytest.mark.gpu
@pytest.mark.parametrize("W", [8, 2])
@pytest.mark.parametrize("net", [HBH, HC])
def test_round_barriers_ragged(W, net, monkeypatch):
    """Case 2: shard 0's tiles stop halfway (at W = 8 rank 0 owns only
    finished tiles for the second half and the barrier's count shrinks); a
    leading and a trailing BARRIER."""
    _plain_knobs(monkeypatch)
    _, m, _ = _trace("ragged")
    assert int((m == C.META_BARRIER).sum()) == 178
    _check("ragged", W, 64, 8, net)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["slot1", "short_batch"])
def test_round_barriers_round_modes(mode, monkeypatch):
    """Case 3: the sized overflow round (GG_ROUND_SLOT=1) and the repeated
    round (GG_ROUND_BATCH0=1,16: the repeat continues at a step > 0 and must
    not apply the release again)."""
    _plain_knobs(monkeypatch)
    if mode == "slot1":
        monkeypatch.setenv("GG_ROUND_SLOT", "1")
    else:
        monkeypatch.setenv("GG_ROUND_BATCH0", "1,16")
    _, stats = _check("hot", 4, 64, 8, HBH)
    if mode == "slot1":
        assert stats["overflow"] > 0, stats
    else:
        assert stats["again"] > 0, stats


@pytest.mark.gpu
@pytest.mark.parametrize("protocol", [C.PROTO_MOSI, C.PROTO_SHL2_MESI])
def test_round_barriers_protocols(protocol, monkeypatch):
    """Case 4: the MOSI and shared-L2 MESI step kernels."""
    _plain_knobs(monkeypatch)
    _check("proto", 4, 64, 8, HC, protocol)


@pytest.mark.gpu
def test_round_barriers_more_tiles_than_a_wave(monkeypatch):
    """Case 5: 128 owned tiles per rank (the tail's tile loop, 64-bit clock max)."""
    _plain_knobs(monkeypatch)
    _check("wide", 2, 256, 8, HC)


@pytest.mark.gpu
@pytest.mark.parametrize("W", [2, 4])
def test_round_barriers_real_fft(W, monkeypatch):
    """Case 6: the reference's fft.C (-p16 -m10), 7 barriers per thread, 4
    shards; the core model over the summed access words."""
    from graphite_amd import backend as B
    from oracle import pyoracle as po
    _plain_knobs(monkeypatch)
    torch = torch_dev()
    got, _ = _check("fft", W, 16, 4, HC)
    _, m, o = _trace("fft")
    cfg = _cfg(16, 4, HC)
    be = B.Backend(cfg)
    try:
        be.core_model_run(to_dev(torch, m, torch.int32), o, to_dev(torch, got[0], torch.int64))
        core = be.core_stats()
    finally:
        be.close()
    assert np.array_equal(core, po.core_model(m, _oracle("fft", 16, 4, HC)[0], o, cfg.frequency_ghz))


RCCL_SCRIPT = r"""
import os, sys, numpy as np, torch, torch.distributed as dist
sys.path.insert(0, %r)
from graphite_amd import config as C, backend as B, coherent as CO
from oracle import pyoracle as po
dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d", world_size=1, rank=0)
torch.cuda.set_device(0)
T, N, K = 64, 200, 8
a, m, o = po.gen_trace(T, N, hot_lines=16)
pos = np.arange(50, N, 50)                       # a BARRIER after every 50 accesses of each tile
a = np.concatenate([np.insert(a[o[t]:o[t + 1]], pos, np.uint64(0)) for t in range(T)])
m = np.concatenate([np.insert(m[o[t]:o[t + 1]], pos, np.uint32(C.META_BARRIER)) for t in range(T)])
o = np.arange(T + 1, dtype=np.uint64) * np.uint64(N + len(pos))
addr = torch.from_numpy(a.view(np.int64)).cuda(); meta = torch.from_numpy(m.view(np.int32)).cuda()
res = []
for mode in ("rccl", "rccl_slot1", "single"):
    os.environ["GG_ROUND_SLOT"] = "1" if mode == "rccl_slot1" else "1024"
    cfg = C.default_config(T, num_shards=K, net_model=C.NET_EMESH_HOP_BY_HOP)
    be = B.Backend(cfg)
    out = torch.zeros(len(a), dtype=torch.int64, device="cuda")
    if mode.startswith("rccl"):
        CO.run_rccl(be, addr, meta, o, out)
    else:
        be.coherent_run(addr, meta, o, out)
    torch.cuda.synchronize()
    st, cc, ri = be.coherent_stats()
    res.append((out.cpu().numpy(), st, cc, be.noc_counters()))
    be.close()
ok = all(np.array_equal(x, y) for r in res[1:] for x, y in zip(res[0], r))
oc = po.OracleCoherent(C.default_config(T, num_shards=K, net_model=C.NET_EMESH_HOP_BY_HOP))
ref = oc.run(a, m, o)
ok = ok and np.array_equal(res[0][0].view(np.uint64), ref) and np.array_equal(res[0][1], oc.tile_stats())
ok = ok and np.array_equal(res[0][3], oc.net_counters())
dist.destroy_process_group()
print("RCCL_BARRIER_RUN_OK" if ok else "RCCL_BARRIER_RUN_MISMATCH")
"""


@pytest.mark.gpu
def test_round_barriers_over_rccl():
    """Case 7: coherent.run_rccl (gg_coherent_run_ranks over a one-rank RCCL
    communicator, in a fresh child process) on case 1's hop-by-hop trace, with
    the default slot and with one-record slots."""
    torch_dev()
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-c", RCCL_SCRIPT % (ROOT, port)], capture_output=True, text=True, timeout=240,
                       env=env)
    assert "RCCL_BARRIER_RUN_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


# ---- case 8: the input conditions, with the oracle alone ------------------
def _releases(m, out, offs, gap_ps=1000):
    """The barrier records grouped by the release they left at: a list of
    (release time, stalls of the tiles released) in time order.  A tile's
    clock right after a barrier record is the release time (the sum of its
    gaps, latencies and stalls up to there)."""
    ev = {}
    for t in range(len(offs) - 1):
        s, e = int(offs[t]), int(offs[t + 1])
        mt, w = m[s:e], out[s:e]
        bar = mt == C.META_BARRIER
        step = np.where(bar, 0, (mt & 0x7FFFFFFF) >> 1).astype(np.uint64) * np.uint64(gap_ps) + (w >> np.uint64(2))
        for clk, stall in zip(np.cumsum(step)[bar], (w >> np.uint64(2))[bar]):
            ev.setdefault(int(clk), []).append(int(stall))
    return sorted(ev.items())


@pytest.mark.parametrize("kind,T,net,protocol,nrel", [
    ("hot", 64, HBH, C.PROTO_MSI, 3), ("hot", 64, HC, C.PROTO_MSI, 3),
    ("ragged", 64, HBH, C.PROTO_MSI, None), ("ragged", 64, HC, C.PROTO_MSI, None),
    ("proto", 64, HC, C.PROTO_MOSI, 3), ("proto", 64, HC, C.PROTO_SHL2_MESI, 3)])
def test_oracle_input_conditions(kind, T, net, protocol, nrel):
    """What the GPU cases rely on: at every release some tile has stalled
    longer than a quantum (so it waited over quantum ends at which the round
    must not release) and some tile 0 ps (the latest arrival); in the ragged
    trace the shard-0 tiles finish before the last release."""
    cfg = _cfg(T, 8, net, protocol)
    a, m, o = _trace(kind)
    out, st, _ = _oracle(kind, T, 8, net, protocol)
    bar = m == C.META_BARRIER
    assert np.all((out[bar] & np.uint64(3)) == C.LVL_SYNC)
    rel = _releases(m, out, o)
    assert sum(len(s) for _, s in rel) == int(bar.sum())
    if nrel is not None:
        assert len(rel) == nrel and all(len(s) == T for _, s in rel)
    for _, stalls in rel:
        assert max(stalls) > cfg.quantum_ns * 1000 and min(stalls) == 0, (max(stalls), min(stalls))
    if kind == "ragged":
        assert int(bar.sum()) == 178
        sh = C.shard_map(T, 8)
        clk = st[:, C.TILE_STATS.index("clock_ps")]
        assert len(rel) >= 3 and int(clk[sh == 0].max()) < rel[-1][0]
        assert len(rel[-1][1]) == int((sh != 0).sum())       # the last barrier's count has shrunk
