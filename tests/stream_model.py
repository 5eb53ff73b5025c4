"""Numpy model of the counter-based stream (include/rg_stream.h), written from the header alone: the one statement of mix,
the chain, u, ix and n that every other model of tests/ imports.  Scalars are Python ints masked to 64 bits; the array forms
are uint64, whose arithmetic wraps as the device's does, and are checked against the scalars in tests/test_stream_cpu.py."""
import numpy as np

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
ROOT3 = 1.7320508075688772
U = np.uint64


# ---- scalars -------------------------------------------------------------------------------------------------------------

def mix64(z):
    z &= M64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z


def chain(seed, *words):
    """h of the header: the seed, then one round per word.  Words are ints of any sign (two's-complement 64-bit words)."""
    h = int(seed) & M64
    for w in words:
        h = mix64(((h ^ (int(w) & M64)) + GOLDEN) & M64)
    return h


def uniform(seed, *words):
    """u: the 53-bit uniform in [0, 1) of the chain."""
    return float(chain(seed, *words) >> 11) * 2.0 ** -53


def ix(k, row, j=0):
    """The index word of a per-tick draw."""
    return ((int(k) << 12) | (int(row) << 2) | int(j)) & M64


def noise(seed, key, draw, purpose, k, row):
    """n: one unit-variance draw, a scalar."""
    u0, u1, u2, u3 = (uniform(seed, key, draw, purpose, ix(k, row, j)) for j in range(4))
    return (((u0 + u1) + (u2 + u3)) - 2.0) * ROOT3


def delay_draw(seed, key, draw, purpose, lo, hi):
    return lo + min(int(float(hi - lo + 1) * uniform(seed, key, draw, purpose, 0)), hi - lo)


# ---- arrays --------------------------------------------------------------------------------------------------------------

def _u64(a):
    return np.asarray(a).astype(U) if not (isinstance(a, np.ndarray) and a.dtype == U) else a


def vmix(z):
    with np.errstate(over="ignore"):
        z = z ^ (z >> U(30))
        z = z * U(0xBF58476D1CE4E5B9)
        z = z ^ (z >> U(27))
        z = z * U(0x94D049BB133111EB)
        return z ^ (z >> U(31))


def vchain(seed, *words):
    """chain on uint64 arrays that broadcast."""
    h = U(int(seed) & M64)
    with np.errstate(over="ignore"):
        for w in words:
            h = vmix((h ^ _u64(w)) + U(GOLDEN))
    return h


def vuniform(seed, *words):
    return (vchain(seed, *words) >> U(11)).astype(np.float64) * 2.0 ** -53


def vnoise(seed, key, draw, purpose, k, row):
    """n on arrays: key, draw, k uint64 (robots), row uint64; all broadcast."""
    base = (_u64(k) << U(12)) | (_u64(row) << U(2))
    u0, u1, u2, u3 = (vuniform(seed, key, draw, purpose, base | U(j)) for j in range(4))
    return (((u0 + u1) + (u2 + u3)) - 2.0) * ROOT3


# ---- the two integer readings of a state row -----------------------------------------------------------------------------

def words(v):
    """A state row's integers as the device reads key and draws: through int64 to uint64."""
    return np.asarray(v, dtype=np.float64).astype(np.int64).astype(U)


def bounded(v, hi):
    """A tick, delay or run row: (uint64) fmin(fmax(v, 0), hi); a NaN is 0."""
    v = np.asarray(v, dtype=np.float64)
    return np.minimum(np.maximum(np.where(np.isnan(v), 0.0, v), 0.0), float(hi)).astype(U)
