"""The pairwise configuration sweep on the GPU (tests/sweep_cases.py): every row
of the case table as a lone gg_coherent_run against the oracle, bit for bit,
and then through the row's driver — legs with snapshot and restore, a trace fed
in windows, an ensemble, the two-rank round — word for word against the lone
run.  A kernel that is wrong only where two settings meet fails here; the
single-axis files (test_gpu_config_space.py and the drivers' own files) say
which axis when one alone is wrong.  The helpers are those files' own."""
import functools

import numpy as np
import pytest

from graphite_amd import config as C
from tests import sweep_cases as S
from tests.gpu_util import torch_dev, to_dev, to_np

pytestmark = pytest.mark.gpu

FINAL = C.RUN_INFO.index("final_quantum")
ERR_UNSUPPORTED = -3
NAMES = ("access words", "tile statistics", "cache counters", "NoC counters", "protocol statistics", "run info",
         "miss types")


def _ro(*xs):
    for x in xs:
        x.setflags(write=False)
    return xs


@functools.lru_cache(maxsize=None)
def _trace(index, n, hot):
    return _ro(*(np.ascontiguousarray(x) for x in S.trace(S.CASES[index], n=n, hot=hot)))


def _tracks(cfg):
    return bool(cfg.l1i_track_miss_types or cfg.l1d_track_miss_types or cfg.l2_track_miss_types)


def _oracle(cfg, a, m, o):
    """The oracle's [access words, tile statistics, cache counters, NoC
    counters, protocol statistics, run info, miss types]."""
    from oracle import pyoracle as po
    oc = po.OracleCoherent(cfg)
    words = oc.run(np.array(a), np.array(m), np.array(o))
    return [words, oc.tile_stats(), oc.cache_counters(), oc.net_counters(), oc.proto_stats(),
            oc.run_info(), oc.miss_types()]


def _same(got, ref, what, fields=NAMES):
    for name, x, y in zip(NAMES, got, ref):
        if name in fields and not np.array_equal(x, y):
            d = np.argwhere(np.asarray(x) != np.asarray(y))
            raise AssertionError("%s: %s differ at %d places, first %s: %s != %s"
                                 % (what, name, len(d), d[0], np.asarray(x)[tuple(d[0])], np.asarray(y)[tuple(d[0])]))


def _fields(cfg):
    """What a run of cfg is compared in: the protocol statistics under MOSI
    (zeros elsewhere on both sides), the miss types where tracked."""
    return tuple(n for n in NAMES if (n != "miss types" or _tracks(cfg)))


def _protocol_compare(cfg):
    if cfg.protocol == C.PROTO_MOSI:
        from tests.test_gpu_mosi import _compare
    elif cfg.protocol in (C.PROTO_SHL2_MSI, C.PROTO_SHL2_MESI):
        from tests.test_gpu_shl2 import _compare
    else:
        from tests.coherent_util import _compare
    return _compare


def _lone(cfg, a, m, o):
    """gg_coherent_run over the whole trace: its state, with the miss types."""
    from tests.test_gpu_trace_windows import _whole
    be, st = _whole(cfg, a, m, o)
    st = st + [be.miss_types() if _tracks(cfg) else np.zeros(0, np.uint64)]
    be.close()
    return st


def _lone_against_oracle(cfg, a, m, o, what, barriers):
    """a. of a case: the protocol's own comparison (its invariants count every
    record as an access, so a trace with BARRIER records goes without it), then
    every output of gg_coherent_run against the oracle's."""
    if not barriers:
        _protocol_compare(cfg)(cfg, np.array(a), np.array(m), np.array(o))
    lone = _lone(cfg, a, m, o)
    ref = _oracle(cfg, a, m, o)
    n = len(C.RUN_INFO)
    _same(lone[:5] + [lone[5][:n], lone[6]], ref[:5] + [ref[5][:n], ref[6]], what + ", lone run against the oracle",
          _fields(cfg))
    if cfg.protocol == C.PROTO_MOSI:
        assert lone[4].any(), "no MOSI event counted"
    return lone


# ---- the drivers -----------------------------------------------------------------------
def _drive_legs(case, cfg, a, m, o, lone):
    from tests.test_gpu_checkpoint import _legs
    F = int(lone[5][FINAL])
    assert F >= 6
    blobs = []
    be, got = _legs(cfg, a, m, o, [1, F // 3, 2 * F // 3], blobs=blobs)
    got = got + [be.miss_types() if _tracks(cfg) else lone[6]]
    be.close()
    print(case.id, "final quantum", F, "pauses at", [q for q, _ in blobs])
    assert len(blobs) == 3
    _same(got, lone, "three pauses in fresh contexts", _fields(cfg))


def _drive_windows(case, cfg, a, m, o, lone):
    from tests.test_gpu_trace_windows import Windowed
    tail = 1 if S.level(case, "trace") in ("barr", "multi") else 0
    w = Windowed(cfg, a, m, o, lambda t, need: need + 8, tail=tail).run(limit=1 << 20)
    got = w.state() + [w.be.miss_types() if _tracks(cfg) else lone[6]]
    w.be.close()
    print(case.id, "hand-overs", w.handovers, "largest min_records", w.max_need, "window ends", w.ends)
    assert w.handovers >= 3
    _same(got, lone, "in windows", _fields(cfg))


def _drive_ensemble(case, cfg, a, m, o, lone):
    """Three instances of the configuration in one set of launches: the case's
    own trace, one of 3 n / 2 and one of n / 2 accesses a tile, each over other
    hot lines; each against its own lone run."""
    from graphite_amd import backend as B
    torch = torch_dev()
    hot = S.hot_lines(case)
    traces = [(a, m, o), _trace(case.index, 3 * case.n // 2, 2 * hot), _trace(case.index, case.n // 2, 3 * hot)]
    lones = [lone] + [_lone(cfg, *t) for t in traces[1:]]
    bes = [B.Backend(cfg) for _ in traces]
    addr = [to_dev(torch, np.array(t[0]), torch.int64) for t in traces]
    meta = [to_dev(torch, np.array(t[1]), torch.int32) for t in traces]
    outs = [torch.zeros(len(t[0]), dtype=torch.int64, device="cuda") for t in traces]
    B.coherent_run_many(bes, addr, meta, [np.array(t[2]) for t in traces], outs)
    torch.cuda.synchronize()
    for i, be in enumerate(bes):
        st, cc, ri = be.coherent_stats()
        got = [to_np(outs[i], np.uint64), st, cc, be.noc_counters(), be.protocol_stats(), ri,
               be.miss_types() if _tracks(cfg) else lones[i][6]]
        _same(got, lones[i], "instance %d of the ensemble" % i, _fields(cfg))
    for be in bes:
        be.close()
    assert len({len(t[0]) for t in traces}) == 3


def _drive_round2(case, cfg, a, m, o, lone, monkeypatch):
    from tests.test_gpu_round import _run_ranks
    torch = torch_dev()
    monkeypatch.setenv("GG_ROUND_SLOT", "1024")
    monkeypatch.delenv("GG_ROUND_BATCH0", raising=False)
    kw = S.config_kw(case)
    cfg_kw = {"T": kw.pop("num_tiles"), "net": kw.pop("net_model"), "protocol": kw.pop("protocol")}
    K = kw.pop("num_shards")
    cfg_kw["config"] = kw
    stats = {"again": 0, "overflow": 0}
    got = _run_ranks(torch, 2, K, cfg_kw, np.array(a), np.array(m), np.array(o), stats)
    print(case.id, "rounds", stats)
    for name, x, y in zip(("access words", "tile statistics", "NoC counters"), got, (lone[0], lone[1], lone[3])):
        assert np.array_equal(x, y), "two ranks: %s differ from the lone run" % name


@pytest.mark.parametrize("case", S.CASES, ids=[c.id for c in S.CASES])
def test_sweep(case, monkeypatch):
    torch_dev()
    cfg = S.config(case)
    a, m, o = _trace(case.index, None, None)
    lone = _lone_against_oracle(cfg, a, m, o, case.id, barriers=S.level(case, "trace") == "barr")
    driver = S.level(case, "driver")
    if driver == "legs":
        _drive_legs(case, cfg, a, m, o, lone)
    elif driver == "win":
        _drive_windows(case, cfg, a, m, o, lone)
    elif driver == "ens":
        _drive_ensemble(case, cfg, a, m, o, lone)
    elif driver == "round2":
        _drive_round2(case, cfg, a, m, o, lone, monkeypatch)
    else:
        assert driver == "lone"


# ---- the excluded pairs ---------------------------------------------------------------------
def _config_pairs():
    return [(a, b) for a, b in S.CONSTRAINTS if "driver" not in (S.LEVEL[a][0], S.LEVEL[b][0])]


@pytest.mark.parametrize("a,b", _config_pairs(), ids=["%s-%s" % p for p in _config_pairs()])
def test_constraint_is_a_refusal(a, b):
    """Every pair of settings in CONSTRAINTS is refused as unsupported, by
    gg_create or by the run's set-up; each level alone is accepted."""
    from graphite_amd import backend as B
    from oracle import pyoracle as po
    torch = torch_dev()
    tr = po.gen_trace(16, 20, hot_lines=8)
    addr, meta = to_dev(torch, tr[0], torch.int64), to_dev(torch, tr[1], torch.int32)

    def run(kw):
        be = B.Backend(C.default_config(16, **kw))
        try:
            be.coherent_run(addr, meta, tr[2], None)
        finally:
            be.close()

    for lab in (a, b):
        run(S.LEVEL[lab][1])
    with pytest.raises(B.GGError) as e:
        run(dict(S.LEVEL[a][1], **S.LEVEL[b][1]))
    assert e.value.code == ERR_UNSUPPORTED, e.value


@pytest.mark.parametrize("T,K", [(16, 1), (12, 3), (20, 5)])
def test_round_refuses_shards_that_do_not_split(T, K):
    from graphite_amd import backend as B
    from oracle import pyoracle as po
    torch = torch_dev()
    a, m, o = po.gen_trace(T, 20, hot_lines=8)
    be = B.Backend(C.default_config(T, num_shards=K))
    try:
        be.coherent_begin(to_dev(torch, a, torch.int64), to_dev(torch, m, torch.int32), o, None)
        with pytest.raises(B.GGError) as e:
            be.round_pack(2, 0, 0)
    finally:
        be.close()
    assert e.value.code == -1 and "do not split" in str(e.value)
@pytest.mark.parametrize("proto", [C.PROTO_SHL2_MSI, C.PROTO_SHL2_MESI])
def test_shared_l2_refuses_l2_miss_types(proto):
    """The run's set-up refuses before any launch: no access word is written."""
    from graphite_amd import backend as B
    from oracle import pyoracle as po
    torch = torch_dev()
    a, m, o = po.gen_trace(16, 50, hot_lines=8)
    be = B.Backend(C.default_config(16, protocol=proto, l1d_track_miss_types=1, l2_track_miss_types=1,
                                    miss_track_lines=1024))
    out = torch.zeros(len(a), dtype=torch.int64, device="cuda")
    try:
        with pytest.raises(B.GGError) as e:
            be.coherent_run(to_dev(torch, a, torch.int64), to_dev(torch, m, torch.int32), o, out)
    finally:
        be.close()
    assert e.value.code == ERR_UNSUPPORTED and "L2 miss types" in str(e.value)
    assert not to_np(out, np.uint64).any()
