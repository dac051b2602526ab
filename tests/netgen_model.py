"""The synthetic network traffic generator (gg_gen_network_traffic, DESIGN.md
§4k) restated in numpy / pure Python: the six destination patterns of the
reference's tests/benchmarks/synthetic_network/synthetic_network.cc:232-359,
the SplitMix64 injection process and the packet fields.  The draws come from
the oracle's oracle_splitmix64_at (oracle/gg_oracle.c:42-45); the vectorised
numpy form used for whole cycle ranges is pinned to it by
tests/test_netgen_model.py."""
import math

import numpy as np

from oracle import pyoracle as po

PATTERNS = ["uniform_random", "bit_complement", "shuffle", "transpose", "tornado", "nearest_neighbor"]
NETPACKET_BYTES = 64
INVALID, RANGE = -1, -4          # GG_ERR_INVALID, GG_ERR_RANGE
_M = (1 << 64) - 1


def splitmix64_at(seed, i):
    return int(po.lib().oracle_splitmix64_at(int(seed) & _M, int(i) & _M))


def splitmix64_range(seed, first, count):
    """oracle_splitmix64_at(seed, first + k) for k < count, as a uint64 array."""
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + (np.arange(first + 1, first + 1 + count, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def mesh(T):
    """(w, h) or None where the reference's computeEMeshTopologyParams asserts."""
    w = int(math.sqrt(1.0 * T))
    h = int(math.ceil(1.0 * T / w))
    return (w, h) if w * h == T else None


def is_pow2(x):
    return x > 0 and x & (x - 1) == 0


def send_matrix_literal(T):
    """uniform_random's matrix as the reference fills it: [time slot][sender],
    each row an LCG run, row i starting where row i - 1 was at its second
    entry."""
    m = [[0] * T for _ in range(T)]
    for slot in range(T):
        m[slot][0] = T // 2 if slot == 0 else m[slot - 1][1]
        for sender in range(1, T):
            m[slot][sender] = (13 * m[slot][sender - 1] + 5) % T
    return m


def orbit(T):
    o = [T // 2]
    for _ in range(2 * T - 1):
        o.append((13 * o[-1] + 5) % T)
    return o


def send_matrix_orbit(T):
    o = orbit(T)
    return [[o[slot + sender] for sender in range(T)] for slot in range(T)]


def uniform_random_valid(T):
    """Every row and every column of the matrix a permutation of the tiles."""
    m = send_matrix_orbit(T)
    full = set(range(T))
    return all(set(r) == full for r in m) and all(set(m[i][j] for i in range(T)) == full for j in range(T))


def fixed_destination(pattern, t, T):
    w, h = mesh(T)
    sx, sy = t % w, t // w
    if pattern == "bit_complement":
        return ~t & (T - 1)
    if pattern == "shuffle":
        nbits = T.bit_length() - 1
        return ((t >> (nbits - 1)) & 1) | ((t << 1) & (T - 1)) if nbits else 0
    if pattern == "transpose":
        return sx * w + sy
    if pattern == "tornado":
        return ((sy + h // 2) % h) * w + (sx + w // 2) % w
    if pattern == "nearest_neighbor":
        return ((sy + 1) % h) * w + (sx + 1) % w
    raise ValueError(pattern)


def destinations(pattern, t, T, N):
    """Destination of packets 0 .. N - 1 of tile t."""
    if pattern == "uniform_random":
        o = orbit(T)
        return np.array([o[(k % T) + t] for k in range(N)], np.uint32)
    return np.full(N, fixed_destination(pattern, t, T), np.uint32)


def check(pattern, T, N, load, packet_bytes=8):
    """The status gg_gen_network_traffic returns before any launch (0 = OK)."""
    if pattern not in PATTERNS or not (0.0 < load <= 1.0) or N == 0 or T == 0:
        return INVALID
    if mesh(T) is None:
        return INVALID
    if pattern in ("bit_complement", "shuffle") and not is_pow2(T):
        return INVALID
    if pattern == "uniform_random" and not uniform_random_valid(T):
        return INVALID
    if T * N >= 1 << 32:
        return RANGE
    if N / load > float(1 << 28):
        return RANGE
    return 0


def cycle_ps(frequency_ghz):
    return int(po.lib().oracle_lat_to_ps(1, frequency_ghz))


def generate(pattern, T, N, load, packet_bytes=8, frequency_ghz=1.0, seed=0):
    """(src, dst, length_bits, time_ps, last_cycle): tile-major, packet k of
    tile t at t * N + k."""
    assert check(pattern, T, N, load, packet_bytes) == 0
    thr = np.uint64(math.ceil(load * 2.0 ** 53))
    one = cycle_ps(frequency_ghz)
    src = np.repeat(np.arange(T, dtype=np.uint32), N)
    dst = np.concatenate([destinations(pattern, t, T, N) for t in range(T)])
    bits = np.full(T * N, (NETPACKET_BYTES + packet_bytes) * 8, np.uint32)
    time = np.zeros(T * N, np.uint64)
    last = np.zeros(T, np.uint64)
    chunk = max(256, int(2 * N / load))
    for t in range(T):
        s_t = splitmix64_at(seed, t)
        cycles, first = [], 0
        while sum(len(c) for c in cycles) < N:
            z = splitmix64_range(s_t, first, chunk)
            cycles.append(first + np.nonzero((z >> np.uint64(11)) < thr)[0])
            first += chunk
        c = np.concatenate(cycles)[:N].astype(np.uint64)
        time[t * N:(t + 1) * N] = c * np.uint64(one)
        last[t] = c[-1]
    return src, dst, bits, time, last
