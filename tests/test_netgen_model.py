"""The synthetic traffic model (tests/netgen_model.py) against the reference's
own invariants, and the checks gg_gen_network_traffic makes on the host before
any launch (no GPU: the calls return before touching the device)."""
import ctypes

import numpy as np
import pytest

from graphite_amd import backend as B
import netgen_model as M

SIZES = [16, 36, 64]


def test_vectorised_draws_equal_the_oracle():
    for seed, first in ((0, 0), (0x9E3779B97F4A7C15, 5), ((1 << 64) - 3, 1000)):
        z = M.splitmix64_range(seed, first, 300)
        assert [int(x) for x in z] == [M.splitmix64_at(seed, first + k) for k in range(300)]


@pytest.mark.parametrize("T", [4] + SIZES)
def test_orbit_form_equals_the_literal_matrix(T):
    assert M.send_matrix_orbit(T) == M.send_matrix_literal(T)


@pytest.mark.parametrize("T", SIZES)
def test_single_destination_patterns_are_permutations(T):
    for p in M.PATTERNS[1:]:
        if M.check(p, T, 1, 1.0) != 0:
            assert p in ("bit_complement", "shuffle") and not M.is_pow2(T)
            continue
        d = sorted(M.fixed_destination(p, t, T) for t in range(T))
        assert d == list(range(T)), p


@pytest.mark.parametrize("T", SIZES)
def test_uniform_random_rows_and_columns_are_permutations(T):
    m = np.array(M.send_matrix_literal(T))
    want = np.arange(T)
    for i in range(T):
        assert np.array_equal(np.sort(m[i]), want) and np.array_equal(np.sort(m[:, i]), want)
    assert M.uniform_random_valid(T)
    # what tile t sends: packet k goes to column t of time slot k % T
    for t in (0, 1, T - 1):
        assert M.destinations("uniform_random", t, T, 2 * T + 3).tolist() == [m[k % T][t] for k in range(2 * T + 3)]


def test_non_square_mesh_patterns_stay_in_range():
    T = 12                                         # 3 x 4
    assert M.mesh(T) == (3, 4)
    for p in ("transpose", "tornado", "nearest_neighbor"):
        assert all(0 <= M.fixed_destination(p, t, T) < T for t in range(T))


def test_injection_rule():
    """Load 1 sends every cycle; the time is cycles x the one-cycle latency
    (667 ps at 1.5 GHz), not a conversion of the whole count."""
    src, dst, bits, t, last = M.generate("transpose", 16, 65, 1.0, 8, 1.5, 7)
    assert t.reshape(16, 65)[3].tolist() == [667 * c for c in range(65)] and last.tolist() == [64] * 16
    assert bits[0] == (64 + 8) * 8 and src.reshape(16, 65)[5].tolist() == [5] * 65
    src, dst, bits, t, last = M.generate("transpose", 16, 100, 0.03, 64, 1.0, 7)
    c = t.reshape(16, 100) // 1000
    assert (np.diff(c.astype(np.int64), axis=1) > 0).all() and np.array_equal(c[:, -1], last)
    assert 1500 < c[:, -1].mean() < 6000 and bits[0] == 1024


def _call(pattern, T, N, load, packet_bytes=8):
    """gg_gen_network_traffic with host arrays in place of device arrays: every
    case here is rejected before the pointers are used."""
    p = B.TrafficParams(pattern, packet_bytes, load, N, 1)
    a = np.zeros(4, np.uint64)
    ptr = a.ctypes.data_as(ctypes.c_void_p)
    return B.load().gg_gen_network_traffic(ctypes.byref(p), T, 1.0, ptr, ptr, ptr, ptr, None, None)


REJECTED = [
    ("uniform_random", 100, 10, 0.5, M.INVALID),       # a column of the matrix is no permutation
    ("bit_complement", 36, 10, 0.5, M.INVALID),
    ("shuffle", 36, 10, 0.5, M.INVALID),
    ("transpose", 32, 10, 0.5, M.INVALID),             # 5 x 7 != 32
    ("transpose", 16, 10, 0.0, M.INVALID),
    ("transpose", 16, 10, 1.5, M.INVALID),
    ("transpose", 16, 0, 0.5, M.INVALID),
    ("transpose", 16, 1 << 28, 1.0, M.RANGE),          # T * N = 2^32
    ("transpose", 16, (1 << 27) + 1, 0.5, M.RANGE),    # N / load > 2^28
    ("transpose", 16, 1000, 1e-6, M.RANGE),
]


@pytest.mark.parametrize("pattern,T,N,load,code", REJECTED)
def test_host_rejections(pattern, T, N, load, code):
    assert M.check(pattern, T, N, load) == code
    assert _call(pattern, T, N, load) == code
    assert B.load().gg_last_error()


def test_unknown_pattern_and_null_arrays_are_invalid():
    assert _call(6, 16, 10, 0.5) == M.INVALID
    p = B.TrafficParams("transpose", 8, 0.5, 10, 1)
    assert B.load().gg_gen_network_traffic(ctypes.byref(p), 16, 1.0, None, None, None, None, None, None) == M.INVALID
    assert B.load().gg_gen_network_traffic(None, 16, 1.0, None, None, None, None, None, None) == M.INVALID
    assert B.load().gg_noc_latency_stats(None, None, None, None) == M.INVALID
    assert B.load().gg_noc_synthetic_run(None, ctypes.byref(p), None, None) == M.INVALID


def test_symbols_and_defaults():
    L = B.load()
    for name in ("gg_traffic_params_default", "gg_gen_network_traffic", "gg_noc_latency_stats", "gg_noc_synthetic_run"):
        assert hasattr(L, name) and name in B.EXPORTS
    p = B.TrafficParams(3, 1, 1.0, 1, 1)
    L.gg_traffic_params_default(ctypes.byref(p))
    assert (p.pattern, p.packet_bytes, p.offered_load, p.packets_per_tile, p.seed) == (0, 8, 0.1, 10000, 0)
    assert B.TRAFFIC_PATTERNS == M.PATTERNS and B.NUM_NLS == 73 and B.NETPACKET_BYTES == M.NETPACKET_BYTES
