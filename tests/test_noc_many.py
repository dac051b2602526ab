"""The CPU side of the NoC ensemble entries: the bindings exist
and the library exports them, and the instance sets of tests/test_gpu_noc_many.py
reach the kernel forms and fall-backs they are built for."""
import ctypes

from graphite_amd import backend as B
import test_gpu_noc_many as G


def test_library_exports_the_many_entries():
    lib = ctypes.CDLL(B.LIB_PATH)
    for name in ("gg_noc_route_batch_many", "gg_noc_synthetic_run_many"):
        assert name in B.EXPORTS and hasattr(lib, name), name
    assert B.load().gg_noc_route_batch_many.restype is ctypes.c_int32 or B.load().gg_noc_route_batch_many.restype is ctypes.c_int


def test_sets_reach_the_kernel_forms_they_are_meant_for():
    """The forms and fall-backs the GPU sets are built for, by the rules of noc_traffic."""
    assert callable(B.noc_route_batch_many) and callable(B.noc_synthetic_run_many)
    th = G.nt.thresholds()
    for name, form in (("hbh16", "pipe"), ("hbh64", "pipe"), ("hbh12", "pipe"), ("sweep33", "sweep"), ("hbm1024", "hbm")):
        for cfg in G.cfgs_of(name):
            assert G.nt.chain_kernel(cfg) == (form, form), name
    T, insts = G.SETS["hbh64"]
    cfgs = G.cfgs_of("hbh64")
    src, dst, bits, _ = insts[4]["batch"]
    assert G.nt.per_source(T, src, dst).max() == th["kPortPk"] + 1 and G.nt.per_destination(T, src, dst).max() == th["kPortPk"] + 1
    src, dst, bits, _ = insts[5]["batch"]
    assert G.nt.per_xchain(T, src, dst).max() == th["kPipePk"] + 1
    assert "pipe" not in G.nt.chain_paths(cfgs[5], src, dst, bits)[0].values()   # beyond kPipePk: a fall-back
    for k in (2, 3):                                  # history_list / basic: chain_staged inside the pipeline kernel
        b = G.batch_of(T, insts[k])
        paths = G.nt.chain_paths(cfgs[k], b[0], b[1], b[2])
        assert set(paths[0].values()) | set(paths[1].values()) == {"staged"}
    # uneven grids: the packet counts of the 16-tile set span 16 .. 1600, blocks of 256 packets
    counts = sorted(16 * i["p"][3] for i in G.SETS["hbh16"][1])
    assert counts[0] == 16 and counts[-1] == 1600 and {16 * n for n in (1, 63, 64, 65, 100)} <= set(counts)
