"""Many NoC batches side by side: gg_noc_route_batch_many and
gg_noc_synthetic_run_many.

Every instance is held against the C oracle, exactly: the three result arrays
and the per-tile counters of noc_route_batch_many on the batches that
tests/netgen_model.py generates (or tests/noc_traffic.py builds), and the 73
words and the counters of noc_synthetic_run_many against the numpy reduction
over the oracle's arrays for the model's packets.  The device generator's
packets stay in scratch of the context and have no getter; a packet that
differed from the model's would change the counters and the words compared
here.  Then: equality with the single calls, the queue state carried from call
to call, n = 1 and the instance order, the error rules, the sweep tool and
gg_replay."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from graphite_amd import config as C
from graphite_amd import backend as B
from oracle import pyoracle as po
import netgen_model as M
import noc_traffic as nt
from gpu_util import torch_dev, to_dev, to_np

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPLAY = os.path.join(ROOT, "graphite_amd", "host", "gg_replay")
SWEEP = os.path.join(ROOT, "tools", "noc_load_sweep.py")
HBH = dict(net_model=C.NET_EMESH_HOP_BY_HOP)
INVALID, UNSUPPORTED, RANGE = -1, -3, -4          # GG_ERR_*
DTYPES = ("int32", "int32", "int32", "int64")


def numpy_stats(src, dst, t, arr, zl, ct):
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


def synth(pattern, load, N, pb=8, seed=0, **cfg_kw):
    """One synthetic instance: config overrides and the traffic parameters."""
    return dict(cfg_kw=cfg_kw, p=(pattern, pb, load, N, seed))


def batch_of(T, inst):
    """The instance's packets on the host (the generator's model, or the explicit batch)."""
    if "batch" in inst:
        return tuple(inst["batch"])
    pattern, pb, load, N, seed = inst["p"]
    cfg = C.default_config(T, **inst["cfg_kw"])
    return tuple(M.generate(pattern, T, N, load, pb, cfg.frequency_ghz, seed)[:4])


def oracle_of(cfg, batches):
    """One oracle object routing the batches in sequence: [(arr, zl, ct)], counters."""
    on = po.OracleNoc(cfg)
    res = [on.route(*b) for b in batches]
    return res, on.counters()


def upload(torch, batch):
    return [to_dev(torch, x, getattr(torch, dt)) for x, dt in zip(batch, DTYPES)]


def outs_for(torch, n):
    return [torch.full((n,), -1, dtype=torch.int64, device="cuda") for _ in range(3)]


def route_many(torch, bes, batches):
    devs = [upload(torch, b) for b in batches]
    outs = [outs_for(torch, len(b[0])) for b in batches]
    st = B.noc_route_batch_many(bes, devs, outs)
    torch.cuda.synchronize()
    return st, [[to_np(x, np.uint64) for x in o] for o in outs]


# ---- the sets of the issue ------------------------------------------------------------------------
def _sets():
    th = nt.thresholds()
    s = {}
    s["hbh16"] = (16, [
        synth("uniform_random", 1.0, 1, 8, 1, **HBH),
        synth("bit_complement", 0.03, 63, 64, 2, **HBH, frequency_ghz=1.5),
        synth("shuffle", 0.5, 64, 8, 3, **HBH, router_delay=2, link_delay=2),
        synth("transpose", 1.0, 65, 64, 4, **HBH, flit_width=32, queue_model_enabled=0),
        synth("tornado", 0.3, 100, 8, 5, **HBH, frequency_ghz=1.5, router_delay=0, link_delay=1, flit_width=128),
        synth("nearest_neighbor", 0.03, 100, 8, 6, **HBH, queue_model_enabled=0, frequency_ghz=1.5),
        synth("uniform_random", 0.5, 100, 64, 7, **HBH, router_delay=3),
        synth("transpose", 0.1, 64, 8, 8, **HBH, flit_width=16, link_delay=3),
    ])
    s["hbh64"] = (64, [
        synth("uniform_random", 0.5, 100, 8, 1, **HBH, max_list_size=100),
        synth("transpose", 0.3, 65, 8, 2, **HBH, max_list_size=3),
        synth("tornado", 0.5, 64, 8, 3, **HBH, queue_model_type=C.QM_HISTORY_LIST),
        synth("shuffle", 0.5, 63, 8, 4, **HBH, queue_model_type=C.QM_BASIC),
        dict(cfg_kw=dict(HBH), batch=nt.port_edge(64, th["kPortPk"] + 1, 9, 20_000_000), reaches="port_over"),
        dict(cfg_kw=dict(HBH), batch=nt.one_chain(64, th["kPipePk"] + 1, 8, 40_000_000), reaches="pipe_over"),
    ])
    s["hbh12"] = (12, [synth(p, 0.5, 65, 8, i, **HBH) for i, p in enumerate(("transpose", "tornado", "nearest_neighbor"))])
    for name, net in (("hop_counter", C.NET_EMESH_HOP_COUNTER), ("magic", C.NET_MAGIC)):
        s[name] = (16, [
            synth("uniform_random", 1.0, 65, 8, 1, net_model=net),
            synth("transpose", 0.03, 1, 64, 2, net_model=net, frequency_ghz=1.5),
            synth("tornado", 0.5, 100, 8, 3, net_model=net, router_delay=2, link_delay=3, flit_width=32),
            synth("shuffle", 0.3, 64, 8, 4, net_model=net),
        ])
    s["sweep33"] = (1089, [dict(cfg_kw=dict(HBH), batch=nt.uniform(1089, 300, 1, 3_000_000)),
                           dict(cfg_kw=dict(HBH, frequency_ghz=1.5, max_list_size=50),
                                batch=nt.uniform(1089, 411, 2, 3_000_000))])
    s["hbm1024"] = (1024, [dict(cfg_kw=dict(HBH, max_list_size=320), batch=nt.uniform(1024, 300, 3, 3_000_000)),
                           dict(cfg_kw=dict(HBH, max_list_size=320, router_delay=2),
                                batch=nt.uniform(1024, 257, 4, 3_000_000))])
    return s


SETS = _sets()


def cfgs_of(name):
    T, insts = SETS[name]
    return [C.default_config(T, **i["cfg_kw"]) for i in insts]


@functools.lru_cache(maxsize=None)
def reference(name):
    """Per instance of a set: its batch, the oracle's arrays and counters for that one batch on a
    fresh network, and the reduction over them.  Computed once, never changed."""
    T, insts = SETS[name]
    out = []
    for cfg, inst in zip(cfgs_of(name), insts):
        b = batch_of(T, inst)
        (res,), ctr = oracle_of(cfg, [b])
        out.append(dict(batch=b, res=res, counters=ctr, stats=numpy_stats(b[0], b[1], b[3], *res)))
    return out


def check_instance(got, counters, ref, what):
    for g, x, nm in zip(got, ref["res"], ("arrival", "zero_load", "contention")):
        np.testing.assert_array_equal(g, x, err_msg="%s: %s" % (what, nm))
    np.testing.assert_array_equal(counters, ref["counters"], err_msg="%s: counters" % what)


# ---- 1. each instance against the oracle ----------------------------------------------------------
@pytest.mark.parametrize("name", list(SETS))
def test_route_many_matches_oracle(name):
    torch = torch_dev()
    ref = reference(name)
    bes = [B.Backend(c) for c in cfgs_of(name)]
    st, got = route_many(torch, bes, [r["batch"] for r in ref])
    assert st == [0] * len(bes)
    for i, be in enumerate(bes):
        check_instance(got[i], be.noc_counters(), ref[i], "%s instance %d" % (name, i))
        be.close()
    if name.startswith("hbh"):
        assert any(r["res"][2].any() for r in ref), "the set is meant to queue somewhere"


SYNTH_SETS = ["hbh16", "hbh64", "hbh12", "hop_counter", "magic"]


def synth_part(name):
    T, insts = SETS[name]
    idx = [i for i, x in enumerate(insts) if "p" in x]
    return idx, [B.TrafficParams(*insts[i]["p"]) for i in idx]


@pytest.mark.parametrize("name", SYNTH_SETS)
def test_synthetic_run_many_matches_oracle(name):
    torch_dev()
    ref, cfgs = reference(name), cfgs_of(name)
    idx, params = synth_part(name)
    bes = [B.Backend(cfgs[i]) for i in idx]
    stats = B.noc_synthetic_run_many(bes, params)
    for be, i, s in zip(bes, idx, stats):
        np.testing.assert_array_equal(s, ref[i]["stats"], err_msg="%s instance %d: stats" % (name, i))
        np.testing.assert_array_equal(be.noc_counters(), ref[i]["counters"], err_msg="%s instance %d: counters" % (name, i))
        be.close()


# ---- 2. equal to the single call ------------------------------------------------------------------
def test_many_equals_single_calls_64_tiles():
    torch = torch_dev()
    name = "hbh64"
    ref, cfgs = reference(name), cfgs_of(name)
    idx, params = synth_part(name)
    many = [B.Backend(cfgs[i]) for i in idx]
    single = [B.Backend(cfgs[i]) for i in idx]
    stats = B.noc_synthetic_run_many(many, params)
    for a, b, p, s in zip(many, single, params, stats):
        np.testing.assert_array_equal(b.noc_synthetic_run(p), s)
        np.testing.assert_array_equal(a.noc_counters(), b.noc_counters())
        assert a.dump_summary() == b.dump_summary()
    # the result arrays: the whole set through route_batch_many against noc_route_batch one by one
    bm = [B.Backend(c) for c in cfgs]
    _, got = route_many(torch, bm, [r["batch"] for r in ref])
    for i, c in enumerate(cfgs):
        b1 = B.Backend(c)
        dev, o = upload(torch, ref[i]["batch"]), outs_for(torch, len(ref[i]["batch"][0]))
        b1.noc_route_batch(*dev, *o)
        torch.cuda.synchronize()
        for g, x in zip(got[i], o):
            np.testing.assert_array_equal(g, to_np(x, np.uint64))
        np.testing.assert_array_equal(bm[i].noc_counters(), b1.noc_counters())
        assert bm[i].dump_summary() == b1.dump_summary()
        b1.close()
    for be in many + single + bm:
        be.close()


# ---- 3. the queue state carries over --------------------------------------------------------------
def test_queue_state_carries_over_and_reset():
    torch = torch_dev()
    T = 16
    cfgs = [C.default_config(T, **HBH), C.default_config(T, **HBH, frequency_ghz=1.5, max_list_size=7),
            C.default_config(T, **HBH, queue_model_type=C.QM_HISTORY_LIST)]
    b1 = [M.generate("uniform_random", T, 65, 0.5, 8, c.frequency_ghz, 10 + i)[:4] for i, c in enumerate(cfgs)]
    b2 = [M.generate("transpose", T, 30 + i, 1.0, 64, c.frequency_ghz, 20 + i)[:4] for i, c in enumerate(cfgs)]
    b3 = M.generate("tornado", T, 40, 0.5, 8, cfgs[1].frequency_ghz, 30)[:4]
    bes = [B.Backend(c) for c in cfgs]
    _, g1 = route_many(torch, bes, b1)
    _, g2 = route_many(torch, bes, b2)
    dev, o = upload(torch, b3), outs_for(torch, len(b3[0]))
    bes[1].noc_route_batch(*dev, *o)
    torch.cuda.synchronize()
    for i, c in enumerate(cfgs):
        res, ctr = oracle_of(c, [b1[i], b2[i]] + ([b3] if i == 1 else []))
        for g, x in zip(g1[i] + g2[i], res[0] + res[1]):
            np.testing.assert_array_equal(g, x)
        if i == 1:
            for g, x in zip(o, res[2]):
                np.testing.assert_array_equal(to_np(g, np.uint64), x)
        np.testing.assert_array_equal(bes[i].noc_counters(), ctr)
    assert any(not np.array_equal(g2[i][2], oracle_of(c, [b2[i]])[0][0][2]) for i, c in enumerate(cfgs)), \
        "the second batch is meant to meet the first one's queues"
    for be in bes:
        be.reset()
    _, g = route_many(torch, bes, b1)
    for i in range(len(cfgs)):
        for a, b in zip(g[i], g1[i]):
            np.testing.assert_array_equal(a, b)
        bes[i].close()


# ---- 4. n = 1 and the order -----------------------------------------------------------------------
def test_one_instance_and_permutation():
    torch = torch_dev()
    name = "hbh16"
    ref, cfgs = reference(name), cfgs_of(name)
    idx, params = synth_part(name)
    be = B.Backend(cfgs[6])
    np.testing.assert_array_equal(B.noc_synthetic_run_many([be], [params[6]])[0], ref[6]["stats"])
    np.testing.assert_array_equal(be.noc_counters(), ref[6]["counters"])
    be.close()
    be = B.Backend(cfgs[6])
    _, got = route_many(torch, [be], [ref[6]["batch"]])
    check_instance(got[0], be.noc_counters(), ref[6], "n = 1")
    be.close()
    perm = [5, 0, 7, 2, 6, 1, 4, 3]
    bes = [B.Backend(cfgs[i]) for i in perm]
    stats = B.noc_synthetic_run_many(bes, [params[i] for i in perm])
    for be, i, s in zip(bes, perm, stats):
        np.testing.assert_array_equal(s, ref[i]["stats"])
        np.testing.assert_array_equal(be.noc_counters(), ref[i]["counters"])
        be.close()
    bes = [B.Backend(cfgs[i]) for i in perm]
    _, got = route_many(torch, bes, [ref[i]["batch"] for i in perm])
    for be, i, g in zip(bes, perm, got):
        check_instance(g, be.noc_counters(), ref[i], "permuted %d" % i)
        be.close()


# ---- 5. errors ------------------------------------------------------------------------------------
def refused(fn, code, *words):
    with pytest.raises(B.GGError) as e:
        fn()
    assert e.value.code == code, str(e.value)
    for w in words:
        assert w in str(e.value), str(e.value)
    return e.value


def test_set_level_rejections_change_nothing():
    torch = torch_dev()
    T = 16
    cfg = C.default_config(T, **HBH)
    b = M.generate("transpose", T, 20, 0.5, 8, 1.0, 1)[:4]
    bes = [B.Backend(cfg) for _ in range(3)]
    route_many(torch, bes, [b] * 3)
    before = [be.noc_counters() for be in bes]
    p = B.TrafficParams("transpose", 8, 0.5, 20, 1)
    dev, out = upload(torch, b), outs_for(torch, len(b[0]))

    def both(ctxs, code, *words):
        n = len(ctxs)
        devs, outs = [dev] * n, [out] * n             # (refused before anything is read or written)
        refused(lambda: B.noc_route_batch_many(ctxs, devs, outs), code, "gg_noc_route_batch_many", *words)
        refused(lambda: B.noc_synthetic_run_many(ctxs, [p] * n), code, "gg_noc_synthetic_run_many", *words)

    class Null:
        h = None
    both([], INVALID, "n == 0")
    both([bes[0]] * (B.MANY_MAX + 1), INVALID, "GG_MANY_MAX")
    both([bes[0], Null(), bes[1]], INVALID, "context 1 is NULL")
    both([bes[0], bes[1], bes[0]], INVALID, "context 2 is context 0 again")
    other = B.Backend(C.default_config(64, **HBH))
    both([bes[0], bes[1], other], INVALID, "context 2", "num_tiles")
    hc = B.Backend(C.default_config(T, net_model=C.NET_EMESH_HOP_COUNTER))
    both([bes[0], hc], INVALID, "context 1", "net_model")
    atac = B.Backend(C.default_config(T, net_model=C.NET_ATAC))
    both([bes[0], bes[1], atac], UNSUPPORTED, "context 2", "ATAC")
    # the pipeline and the HBM-queue form on one mesh (32 x 32: the side fits the pipeline, a list of 320 does not fit LDS)
    big = [B.Backend(C.default_config(1024, **HBH)), B.Backend(C.default_config(1024, **HBH, max_list_size=320))]
    assert nt.chain_kernel(big[0].cfg) == ("pipe", "pipe") and nt.chain_kernel(big[1].cfg) == ("hbm", "hbm")
    both(big, INVALID, "context 1", "kernel form")
    for be, c in zip(bes, before):
        np.testing.assert_array_equal(be.noc_counters(), c)
    for be in bes + big + [other, hc, atac]:
        be.close()


def test_pipeline_and_sweep_forms_do_not_mix():
    """A 33-position side takes the position sweep; no mesh of the same tile count takes the
    pipeline, so the two forms differ in num_tiles first.  The form check itself is reached with the
    HBM form (test_set_level_rejections_change_nothing); here the pair is refused by index."""
    torch_dev()
    a, b = B.Backend(C.default_config(1024, **HBH)), B.Backend(C.default_config(1089, **HBH))
    assert nt.chain_kernel(a.cfg)[0] == "pipe" and nt.chain_kernel(b.cfg)[0] == "sweep"
    p = B.TrafficParams("transpose", 8, 0.5, 2, 1)
    refused(lambda: B.noc_synthetic_run_many([a, b], [p, p]), INVALID, "context 1")
    a.close()
    b.close()


def test_instance_errors_fail_alone():
    torch = torch_dev()
    # a load of 1.5 on 16 tiles; bit_complement on 12 tiles
    for T, bad in ((16, B.TrafficParams("transpose", 8, 1.5, 30, 1)), (12, B.TrafficParams("bit_complement", 8, 0.5, 30, 1))):
        cfg = C.default_config(T, **HBH)
        good = [("transpose", 8, 0.5, 30, 2), ("tornado", 8, 1.0, 65, 3)]
        params = [B.TrafficParams(*good[0]), bad, B.TrafficParams(*good[1])]
        bes = [B.Backend(cfg) for _ in params]
        e = refused(lambda: B.noc_synthetic_run_many(bes, params), INVALID)
        assert e.statuses == [0, INVALID, 0]
        for k, g in ((0, good[0]), (2, good[1])):
            bt = M.generate(g[0], T, g[3], g[2], g[1], cfg.frequency_ghz, g[4])[:4]
            (res,), ctr = oracle_of(cfg, [bt])
            np.testing.assert_array_equal(e.stats[k], numpy_stats(bt[0], bt[1], bt[3], *res))
            np.testing.assert_array_equal(bes[k].noc_counters(), ctr)
        assert not bes[1].noc_counters().any()
        for be in bes:
            be.close()
    # a destination equal to num_tiles: the deferred range error of that context alone; an empty batch
    T = 16
    cfg = C.default_config(T, **HBH)
    ok = [M.generate("uniform_random", T, 40, 0.5, 8, 1.0, s)[:4] for s in (1, 2)]
    badb = [x.copy() for x in ok[0]]
    badb[1][5] = T
    empty = tuple(x[:0] for x in ok[0])
    bes = [B.Backend(cfg) for _ in range(4)]
    st, got = route_many(torch, bes, [ok[0], badb, empty, ok[1]])
    assert st == [0, 0, 0, 0]
    with pytest.raises(B.GGError) as e:
        bes[1].noc_counters()
    assert e.value.code == RANGE
    for k, bt in ((0, ok[0]), (3, ok[1])):
        (res,), ctr = oracle_of(cfg, [bt])
        for g, x in zip(got[k], res):
            np.testing.assert_array_equal(g, x)
        np.testing.assert_array_equal(bes[k].noc_counters(), ctr)
    assert not bes[2].noc_counters().any()
    # a NULL output pointer with packets is that instance's GG_ERR_INVALID
    dev = [upload(torch, b) for b in (ok[0], ok[1])]
    pks = (B._Packets * 2)(*[B._Packets(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[0].numel())
                            for d in dev])
    o = outs_for(torch, len(ok[1][0]))
    pos = (B._PacketOut * 2)(B._PacketOut(None, None, None), B._PacketOut(o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr()))
    import ctypes
    fresh = [B.Backend(cfg) for _ in range(2)]
    stv = (ctypes.c_int * 2)()
    rc = B.load().gg_noc_route_batch_many((ctypes.c_void_p * 2)(*[b.h for b in fresh]), 2, pks, pos, stv, None)
    torch.cuda.synchronize()
    assert rc == INVALID and list(stv) == [INVALID, 0]
    (res,), ctr = oracle_of(cfg, [ok[1]])
    np.testing.assert_array_equal(to_np(o[0], np.uint64), res[0])
    np.testing.assert_array_equal(fresh[1].noc_counters(), ctr)
    assert not fresh[0].noc_counters().any()
    for be in bes + fresh:
        be.close()


# ---- 6. the tool and replay -----------------------------------------------------------------------
def test_sweep_tool_many_prints_the_same_points():
    torch_dev()
    base = [sys.executable, SWEEP, "--tiles", "16", "--patterns", "transpose,uniform_random", "--loads", "0.05,0.3",
            "--models", "hop_by_hop", "--packets", "64", "--reps", "1"]
    timing = ("generate_ms", "route_ms", "reduce_ms", "many", "reps")

    def points(extra):
        out = subprocess.run(base + extra, capture_output=True, text=True, check=True, timeout=300).stdout
        rows = [json.loads(x) for x in out.splitlines()]
        return [{k: v for k, v in r.items() if k not in timing} for r in rows if "pattern" in r], \
               [r for r in rows if "sweep_ms" in r]
    one, none = points([])
    many, sweep = points(["--many", "--compare-loop"])
    assert len(one) == 4 and one == many and not none
    assert len(sweep) == 1 and sweep[0]["points"] == 4 and sweep[0]["sweep_ms"] > 0 and sweep[0]["loop_ms"] > 0


def test_replay_synthetic_network_with_two_loads():
    torch_dev()
    if not os.path.exists(REPLAY):
        pytest.fail("gg_replay is not built")
    base = [REPLAY, "--tiles", "16", "--net", "hop_by_hop", "--synthetic-network", "tornado", "--packets", "50", "--seed", "3"]

    def run(load):
        return subprocess.run(base + ["--load", load], capture_output=True, text=True, check=True, timeout=120).stdout
    a, b, both = run("0.1"), run("0.6"), run("0.1,0.6")
    assert a != b and a.count("Synthetic Network:") == 1
    assert both == a + b
