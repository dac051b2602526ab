"""The synthetic_memory benchmark's instruction stream restated in Python and
numpy (tests/benchmarks/synthetic_memory/synthetic_memory.cc in
the reference): what gg_gen_memory_traffic must produce, bit for bit.

The address map is drawn with this machine's glibc through ctypes (srandom /
random, the functions the reference calls).  The three per-tile streams are
drand48_r's 48-bit LCG in Python integers; tests/test_memgen_model.py pins it
against glibc's srand48_r / drand48_r.  Every float step goes through
np.float32 in the reference's order."""
import ctypes
import ctypes.util
import functools

import numpy as np

INVALID, RANGE, STATE = -1, -4, -5
LCG_A, LCG_C, MASK48 = 0x5DEECE66D, 0xB, (1 << 48) - 1
NON_MEMORY, RO_READ, RW_READ, RW_WRITE, PRIV_READ, PRIV_WRITE = range(6)
MAX_LIST = 32768
RAND_MAX = 2147483647

_libc = ctypes.CDLL(ctypes.util.find_library("c") or "libc.so.6")
_libc.random.restype = ctypes.c_long
_libc.srandom.argtypes = [ctypes.c_uint]


class ModelError(Exception):
    def __init__(self, code, msg, where=None):
        super().__init__(msg)
        self.code = code
        self.where = where               # (tile, instruction) of a draw that names no type


@functools.lru_cache(maxsize=None)
def lcg_states(seed, n):
    """X_1 .. X_n of drand48_r after srand48_r(seed): np.uint64 (shared: do not write to it)."""
    x = ((seed & 0xFFFFFFFF) << 16) | 0x330E
    out = np.empty(n, np.uint64)
    for i in range(n):
        x = (LCG_A * x + LCG_C) & MASK48
        out[i] = x
    return out


def uniform(states):
    """drand48_r's result: X * 2^-48, exact in double."""
    return states.astype(np.float64) * np.float64(2.0 ** -48)


def derive(p):
    """(frac_ro, cum[6]) as initializeGlobalVariables computes them, in float."""
    pr = [np.float32(x) for x in p.probability]
    den = np.float32(np.float32(pr[1] + pr[2]) + pr[3])
    frac_ro = np.float32(pr[1] / den) if den > 0 else np.float32(0)     # departure 2: 0 / 0 is 0
    cum = [pr[0]]
    for i in range(1, 6):
        cum.append(np.float32(pr[i] + cum[i - 1]))
    return frac_ro, np.array(cum, np.float32)


def ro_boundary(p):
    """Shared lines below this index are read-only."""
    return int(np.float32(derive(p)[0] * np.float32(p.num_shared_addresses)))


def address_map(p, T, line):
    """computeSharedAddressToThreadMapping: (read-only lists, read-write lists),
    one Python list of byte addresses per tile, in push order."""
    shift = int(line).bit_length() - 1
    bound = ro_boundary(p)
    ro, rw = [[] for _ in range(T)], [[] for _ in range(T)]
    _libc.srandom(p.map_seed)
    for i in range(p.num_shared_addresses):
        for j in range(p.degree_of_sharing):
            r = _libc.random()
            tid = int(np.float32(np.float32(np.float32(r) / np.float32(RAND_MAX)) * np.float32(T)))
            if tid >= T:
                raise ModelError(STATE, "map draw names tile %d of %d" % (tid, T))
            (ro if i < bound else rw)[tid].append(i << shift)
    return ro, rw


def check(p, T, line):
    """The rejections that need no draw, in gg_gen_memory_traffic's order of kinds."""
    pow2 = lambda x: x > 0 and x & (x - 1) == 0
    pr = [float(x) for x in p.probability]
    if T == 0 or (p.num_threads and p.num_threads != T) or not pow2(line) or not pow2(p.num_shared_addresses) \
            or (p.num_private_addresses and not pow2(p.num_private_addresses)) or p.degree_of_sharing > T \
            or any(not (0.0 <= x <= 1.0) for x in pr) or p.instructions_per_tile == 0 \
            or (p.num_private_addresses == 0 and np.float32(np.float32(pr[4]) + np.float32(pr[5])) > 0):
        raise ModelError(INVALID, "invalid")
    if (p.num_shared_addresses.bit_length() - 1) + (line.bit_length() - 1) > 30 \
            or T * p.num_private_addresses >= 1 << 31 or p.instructions_per_tile >= 1 << 31:
        raise ModelError(RANGE, "range")


def generate(p, T, line=64):
    """The whole trace.  Returns a dict: tile_offsets [T + 1], addr, meta,
    tail [T], type_counts [T][6] (uint64 / uint32 as the ABI's), and skipped [T]:
    the shared instructions that found their list empty."""
    check(p, T, line)
    N = int(p.instructions_per_tile)
    shift = line.bit_length() - 1
    log_shared = p.num_shared_addresses.bit_length() - 1
    _, cum = derive(p)
    ro, rw = address_map(p, T, line)
    addrs, metas, offs = [], [], [0]
    tail = np.zeros(T, np.uint64)
    counts = np.zeros((T, 6), np.uint64)
    skipped = np.zeros(T, np.uint64)
    for t in range(T):
        X = lcg_states(p.seed_base + t, N)
        u = uniform(X)
        f = u.astype(np.float32)                                     # Random<float>::next(1): (float)(u * 1.0f)
        below = f[:, None] < cum[None, :]
        if not below.any(axis=1).all():
            raise ModelError(STATE, "a draw names no type", (t, int(np.argmin(below.any(axis=1)))))
        ty = below.argmax(axis=1)                                    # the first i with random_num < cum[i]
        counts[t] = np.bincount(ty, minlength=6)
        is_ro = (ty == RO_READ) & (len(ro[t]) > 0)
        is_rw = ((ty == RW_READ) | (ty == RW_WRITE)) & (len(rw[t]) > 0)
        is_pr = (ty == PRIV_READ) | (ty == PRIV_WRITE)
        skipped[t] = int(((ty == RO_READ) | (ty == RW_READ) | (ty == RW_WRITE)).sum() - is_ro.sum() - is_rw.sum())
        a = np.zeros(N, np.uint64)
        for mask, lst in ((is_ro, ro[t]), (is_rw, rw[t])):
            n = int(mask.sum())
            if n:
                if len(lst) > MAX_LIST:
                    raise ModelError(STATE, "tile %d draws from a list of %d entries" % (t, len(lst)))
                # the stream was seeded like the type stream: its draws are X_1, X_2, ...
                idx = (u[:n] * np.float64(len(lst))).astype(np.int64)        # Random<int>::next: (int)(u * size)
                a[mask] = np.array(lst, np.uint64)[idx]
        n = int(is_pr.sum())
        if n:
            k = np.arange(n, dtype=np.uint64) % np.uint64(p.num_private_addresses)
            a[is_pr] = np.uint64(1 << (log_shared + shift)) + ((np.uint64(t * p.num_private_addresses) + k) << np.uint64(shift))
        acc = is_ro | is_rw | is_pr
        nm_before = np.concatenate(([0], np.cumsum(ty == NON_MEMORY)))        # NON_MEMORY among instructions < i
        pos = np.flatnonzero(acc)
        before = nm_before[pos]
        gap = np.diff(np.concatenate(([0], before)))
        wr = (ty[pos] == RW_WRITE) | (ty[pos] == PRIV_WRITE)
        addrs.append(a[pos])
        metas.append((gap.astype(np.uint32) << np.uint32(1)) | wr.astype(np.uint32))
        tail[t] = int(nm_before[N]) - (int(before[-1]) if len(pos) else 0)
        offs.append(offs[-1] + len(pos))
    return dict(tile_offsets=np.array(offs, np.uint64),
                addr=np.concatenate(addrs).astype(np.uint64) if addrs else np.zeros(0, np.uint64),
                meta=np.concatenate(metas).astype(np.uint32) if metas else np.zeros(0, np.uint32),
                tail=tail, type_counts=counts, skipped=skipped)


def numpy_stats(meta, out, NUM_MLS=83, HIST=18):
    """The first ten words and the histogram of gg_mem_latency_stats from host arrays."""
    s = np.zeros(NUM_MLS, np.uint64)
    keep = meta != np.uint32(0xFFFFFFFF)
    m, w = meta[keep], out[keep]
    lat, lvl = w >> np.uint64(2), w & np.uint64(3)
    s[0], s[1], s[2] = len(m), int((m & 1 == 0).sum()), int((m & 1 == 1).sum())
    for k, level in ((3, 0), (5, 1), (7, 2)):
        s[k], s[k + 1] = int((lvl == level).sum()), int(lat[lvl == level].sum())
    s[9] = int(lat.max()) if len(lat) else 0
    for x in lat:
        s[HIST + int(x).bit_length()] += np.uint64(1)
    return s
