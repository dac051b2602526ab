"""bench.py's command line and --dump-outputs: a plain run is the headline
alone (--full off by default), and the dump holds what the timed path
computed, the same from run to run and equal to the oracle's."""
import argparse
import os
import sys

import numpy as np
import pytest

import bench


def test_plain_run_is_the_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.gpus, a.steps, a.warmup, a.full, a.dump_outputs) == (1, 7, 2, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d"
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse()


def test_dump_outputs_format_and_budget(tmp_path, monkeypatch):
    big = np.arange(50000, dtype=np.uint64) * np.uint64(3)
    small = np.arange(24, dtype=np.uint64).reshape(2, 3, 4)
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 1 << 16)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small})
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["big.npy", "small.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 1 << 16
    s = np.load(tmp_path / "a" / "small.npy")
    assert s.dtype == np.float64 and np.array_equal(s, small)
    b = np.load(tmp_path / "a" / "big.npy")
    assert b.dtype == np.float64 and 0 < b.size < big.size
    # a sample of the array's own elements, in index order, the same in every run
    assert np.all(np.diff(b) > 0) and np.all(b % 3 == 0) and b.max() <= float(big.max())
    assert np.array_equal(b, np.load(tmp_path / "b" / "big.npy"))


@pytest.mark.gpu
def test_dump_holds_the_timed_paths_outputs(tmp_path):
    from graphite_amd import config as C
    from oracle import pyoracle as po
    from tests.gpu_util import torch_dev
    torch = torch_dev()
    dev = torch.device("cuda", 0)
    T, N, H, K, net = 64, 60, 16, 8, C.NET_EMESH_HOP_BY_HOP
    args = argparse.Namespace(cpu_threads=1)
    res = []
    for d, steps in (("a", 2), ("b", 1)):
        res.append(bench.coherent_run(args, T, N, H, K, net, 1, 0, dev, steps, 1, False, False,
                                      kernel_profile=False, dump=str(tmp_path / d)))
    assert "bit_exact_checked" not in res[0] and res[0]["kernels"] == {}      # no check, no profile run
    names = ["access_words", "cache_counters", "noc_counters", "run_info", "tile_stats"]
    assert sorted(os.listdir(tmp_path / "a")) == [n + ".npy" for n in names]
    got = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in names}
    for n in names:
        assert got[n].dtype == np.float64
        np.testing.assert_array_equal(got[n], np.load(tmp_path / "b" / (n + ".npy")))
    addr, meta, offs = bench.coherent_workload(T, N, H, dev)
    oc = po.OracleCoherent(C.default_config(T, num_shards=K, net_model=net))
    ref = oc.run(addr.cpu().numpy().view(np.uint64), meta.cpu().numpy().view(np.uint32), offs)
    for n, x in (("access_words", ref), ("tile_stats", oc.tile_stats()), ("cache_counters", oc.cache_counters()),
                 ("noc_counters", oc.net_counters())):
        assert int(x.max()) < 1 << 53
        np.testing.assert_array_equal(got[n], x.astype(np.float64))
    assert got["run_info"][C.RUN_INFO.index("quanta")] == res[0]["quanta"]
