"""The state digest of include/lbm_d2q9_f64_digest.h restated in numpy, for tests/test_f64_digest_host.py and tests/test_f64_digest.py:
the definition's five lines on uint64 arrays, whose arithmetic wraps modulo 2^64.  Nothing of the library is used here."""
import numpy as np

GOLDEN_RATIO, MIX1, MIX2 = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)
MASK = (1 << 64) - 1

# bit patterns a digest must tell apart and no arithmetic instruction may touch: quiet and signalling NaNs with payloads, both zeros,
# the smallest and the largest denormal, both infinities, the largest finite double and its negative
EDGE_BITS = np.array([0x7FF8000000000001, 0xFFF4000000ABCDEF, 0x7FF0000000000001, 0xFFF8000000000000, 0x0000000000000000,
                      0x8000000000000000, 0x0000000000000001, 0x800FFFFFFFFFFFFF, 0x7FF0000000000000, 0xFFF0000000000000,
                      0x7FEFFFFFFFFFFFFF, 0xFFEFFFFFFFFFFFFF], np.uint64)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def row_digests(cells, nx, y0=0):
    """uint64 (rows,): the digests of AoS cells (9 doubles per cell, x fastest) that are global rows [y0, y0 + rows) of a grid nx wide."""
    b = bits(cells).reshape(-1, nx * 9)
    first = np.uint64((y0 * nx * 9) & MASK)                                   # idx of the first value: (y0 * nx + 0) * 9 + 0
    idx = first + np.arange(b.size, dtype=np.uint64).reshape(b.shape)         # value number i of the state is idx first + i
    z = b ^ (idx * GOLDEN_RATIO)
    z = (z ^ (z >> np.uint64(30))) * MIX1
    z = (z ^ (z >> np.uint64(27))) * MIX2
    return (z ^ (z >> np.uint64(31))).sum(axis=1, dtype=np.uint64)


def digest(cells, nx, y0=0):
    return int(row_digests(cells, nx, y0).sum(dtype=np.uint64))


def edge_state(nx, ny, seed=5):
    """(ny, nx, 9) doubles: random bit patterns (so NaNs of every payload, denormals and huge values among ordinary numbers) with
    EDGE_BITS written over values spread through every row."""
    rng = np.random.default_rng(seed)
    b = rng.integers(0, 1 << 64, size=ny * nx * 9, dtype=np.uint64)
    b[rng.random(b.size) < 0.25] &= np.uint64(0x800FFFFFFFFFFFFF)             # a quarter of them denormals or zeros
    stride = max(1, b.size // (4 * EDGE_BITS.size) - 1)
    for rep in range(4):
        at = (rep * EDGE_BITS.size + np.arange(EDGE_BITS.size)) * stride
        b[at[at < b.size]] = EDGE_BITS[:np.count_nonzero(at < b.size)]
    return b.view(np.float64).reshape(ny, nx, 9)
