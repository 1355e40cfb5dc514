"""numpy restatement of the training-batch front (include/nerfail_hip.h, ABI 13): the index shuffle P(key, m) of
nerfail_amd/csrc/index_shuffle.h, vectorised over the indices in uint64 arithmetic masked to 32 bits, and the map from a
population index to (slot, row, column). tests/test_batch_ref.py checks its properties on the CPU; tests/test_hip_train_batch.py
holds the kernels to it bit for bit."""
import numpy as np

ROUNDS = 6
M32 = np.uint64(0xFFFFFFFF)
GOLDEN = 0x9E3779B9


def mix32(h):
    """murmur3's 32-bit finaliser on a uint64 array holding 32-bit values."""
    h = h & M32
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & M32
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & M32
    h ^= h >> np.uint64(16)
    return h


def half_bits(m):
    """Half the width of the network: the smallest half >= 1 with 4^half >= m."""
    half = 1
    while half < 16 and (1 << (2 * half)) < m:
        half += 1
    return half


def round_keys(key):
    key = int(key) & 0xFFFFFFFFFFFFFFFF
    lo, hi = np.uint64(key & 0xFFFFFFFF), key >> 32
    return [mix32(np.array([lo], np.uint64) ^ mix32(np.array([(hi + (r + 1) * GOLDEN) & 0xFFFFFFFF], np.uint64)))[0]
            for r in range(ROUNDS)]


def shuffle(key, m, first=0, n=None, return_walk=False):
    """P(key, m)(first + j) for j < n as int64 (n None: the rest of the permutation); with return_walk also the largest number
    of times the network was applied to one element."""
    m = int(m)
    n = m - first if n is None else n
    assert 1 <= m <= 1 << 31 and 0 <= first and 0 <= n <= m - first
    half = np.uint64(half_bits(m))
    mask = (np.uint64(1) << half) - np.uint64(1)
    ks = round_keys(key)
    x = np.arange(first, first + n, dtype=np.uint64)
    todo = np.ones(n, bool)
    walk = 0
    while todo.any():
        v = x[todo]
        L, R = v >> half, v & mask
        for k in ks:
            L, R = R, L ^ (mix32(R ^ k) & mask)
        x[todo] = (L << half) | R
        todo = x >= np.uint64(m)
        walk += 1
    out = x.astype(np.int64)
    return (out, walk) if return_walk else out


def population(q, wh, ww, row0=0, col0=0, view_ids=None, view0=0):
    """(view, row, column) of population indices q: slot q // (wh ww), row row0 + (q % (wh ww)) // ww, column col0 + q % ww."""
    q = np.asarray(q, np.int64)
    slot, rem = q // (wh * ww), q % (wh * ww)
    view = np.asarray(view_ids, np.int64)[slot] if view_ids is not None else view0 + slot
    return view, row0 + rem // ww, col0 + rem % ww
