"""The synthetic memory model (tests/memgen_model.py) against glibc's drand48_r
and the benchmark's own invariants, and the reference's three input files as
fixtures (no GPU)."""
import ctypes
import os

import numpy as np
import pytest

from graphite_amd import config as C
import memgen_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "synthetic_memory")
INPUT_64 = dict(num_threads=64, degree_of_sharing=1, num_shared_addresses=1024, num_private_addresses=256,
                instructions_per_tile=10000)
PROBS_64 = (0.7, 0.025, 0.060, 0.015, 0.14, 0.06)


class _Drand48Data(ctypes.Structure):
    _fields_ = [("x", ctypes.c_ushort * 3), ("old_x", ctypes.c_ushort * 3), ("c", ctypes.c_ushort),
                ("init", ctypes.c_ushort), ("a", ctypes.c_ulonglong)]


def test_lcg_equals_glibc_drand48_r():
    libc = M._libc
    libc.srand48_r.argtypes = [ctypes.c_long, ctypes.POINTER(_Drand48Data)]
    libc.drand48_r.argtypes = [ctypes.POINTER(_Drand48Data), ctypes.POINTER(ctypes.c_double)]
    for seed in (0, 1, 63, 1023, 0x12345678, (1 << 32) + 5):
        buf, r = _Drand48Data(), ctypes.c_double()
        assert libc.srand48_r(seed, ctypes.byref(buf)) == 0
        want = []
        for _ in range(1000):
            assert libc.drand48_r(ctypes.byref(buf), ctypes.byref(r)) == 0
            want.append(r.value)
        assert M.uniform(M.lcg_states(seed, 1000)).tolist() == want


@pytest.mark.parametrize("name,T,N,degree", [("input.64", 64, 10000, 1), ("input.1024", 1024, 100000, 1),
                                             ("input.test", 64, 100000, 64)])
def test_fixture_files_parse(name, T, N, degree):
    p = C.MemTrafficParams.from_input_file(os.path.join(GOLDEN, name))
    assert (p.num_threads, p.instructions_per_tile, p.degree_of_sharing) == (T, N, degree)
    assert abs(sum(p.probability) - 1.0) < 1e-6
    assert C.MemTrafficParams.from_input_file(os.path.join(GOLDEN, name), ns=4).degree_of_sharing == 4
    if name == "input.64":
        d = C.MemTrafficParams()
        for f, _ in C.MemTrafficParams._fields_:
            a, b = getattr(p, f), getattr(d, f)
            assert (tuple(a) == tuple(b)) if f == "probability" else (a == b), f
        M.check(p, 64, 64)


def test_derived_values_of_input_64():
    p = C.MemTrafficParams()
    frac, cum = M.derive(p)
    assert frac == np.float32(0.25) and M.ro_boundary(p) == 256
    assert cum[5] == np.float32(0.99999994)          # the sequential float adds stop short of 1
    assert M.derive(p.replace(probability=(1, 0, 0, 0, 0, 0)))[0] == 0     # 0 / 0 is 0 here


@pytest.mark.parametrize("T,shared,degree", [(64, 1024, 1), (64, 16, 1), (16, 128, 16), (36, 64, 3)])
def test_map_lists(T, shared, degree):
    p = C.MemTrafficParams(T, degree, shared, 256, 100, PROBS_64)
    ro, rw = M.address_map(p, T, 64)
    assert sum(map(len, ro)) + sum(map(len, rw)) == shared * degree
    bound = int(np.float32(M.derive(p)[0] * np.float32(shared)))
    assert bound == shared // 4
    assert sum(map(len, ro)) == bound * degree
    assert all(a >> 6 < bound for lst in ro for a in lst) and all(a >> 6 >= bound for lst in rw for a in lst)
    # srandom(1) restarts the sequence: the map does not depend on what was drawn before
    M._libc.random()
    assert M.address_map(p, T, 64) == (ro, rw)


def test_the_16_address_map_has_empty_lists_and_a_duplicate():
    """The case tests/test_gpu_memgen.py relies on: most tiles take the empty-list path."""
    p = C.MemTrafficParams(64, 1, 16, 256, 100, PROBS_64)
    ro, rw = M.address_map(p, 64, 64)
    holders = [t for t in range(64) if ro[t] or rw[t]]
    assert 0 < len(holders) < 16 and sum(map(len, ro)) == 4
    assert any(len(ro[t]) + len(rw[t]) > 1 for t in holders)


@pytest.mark.parametrize("kw", [dict(), dict(num_shared_addresses=16), dict(num_private_addresses=4),
                                dict(probability=(0.97, 0.005, 0.005, 0.005, 0.01, 0.005), instructions_per_tile=50)])
def test_trace_accounting(kw):
    T = 16
    p = C.MemTrafficParams(**dict(INPUT_64, num_threads=T, instructions_per_tile=3000)).replace(**kw)
    N = p.instructions_per_tile
    g = M.generate(p, T)
    assert (g["type_counts"].sum(axis=1) == N).all()
    o = g["tile_offsets"].astype(np.int64)
    base = 1 << (p.num_shared_addresses.bit_length() - 1 + 6)
    for t in range(T):
        meta, addr = g["meta"][o[t]:o[t + 1]], g["addr"][o[t]:o[t + 1]]
        recs = o[t + 1] - o[t]
        gaps = int((meta >> 1).sum())
        assert gaps + int(g["tail"][t]) == int(g["type_counts"][t, 0])
        assert gaps + int(g["tail"][t]) + int(g["skipped"][t]) + recs == N
        priv = addr[addr >= base].astype(np.int64)
        k = np.arange(len(priv)) % p.num_private_addresses
        assert (priv == base + ((t * p.num_private_addresses + k) << 6)).all()
        assert (addr[addr < base] >> 6 < p.num_shared_addresses).all()
        assert recs - len(priv) + int(g["skipped"][t]) == int(g["type_counts"][t, 1:4].sum())
        assert (addr & 63 == 0).all()


def test_model_rejections():
    ok = C.MemTrafficParams(**dict(INPUT_64, num_threads=16))
    for code, kw in ((M.INVALID, dict(num_shared_addresses=24)), (M.INVALID, dict(num_shared_addresses=0)),
                     (M.INVALID, dict(num_private_addresses=3)), (M.INVALID, dict(degree_of_sharing=17)),
                     (M.INVALID, dict(instructions_per_tile=0)), (M.INVALID, dict(num_private_addresses=0)),
                     (M.RANGE, dict(num_shared_addresses=1 << 25)), (M.RANGE, dict(num_private_addresses=1 << 27)),
                     (M.RANGE, dict(instructions_per_tile=1 << 31))):
        with pytest.raises(M.ModelError) as e:
            M.check(ok.replace(**kw), 16, 64)
        assert e.value.code == code, kw
    with pytest.raises(M.ModelError) as e:
        M.generate(ok.replace(probability=(0.25, 0.05, 0.05, 0.05, 0.05, 0.05), instructions_per_tile=64), 16)
    assert e.value.code == M.STATE and e.value.where[0] == 0
