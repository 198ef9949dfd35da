"""Seeds and passes of an ensemble of K keyed realisations per slice (ResidualDiffusion.sample_ensemble).  Pure numpy, no GPU.

A replica is an ordinary slice of the samplers with a seed of its own: x_T and the ancestral sampler's step noise are functions of
(seed, step, pixel) alone (fd_keyed_normal), so replica k of a slice is the same image in any batch, on any rank and stream.
"""
import numpy as np

_M64 = (1 << 64) - 1
_GOLDEN, _MUL1, _MUL2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
_REPLICA = 0xD1B54A32D192ED03          # odd: k -> k * _REPLICA mod 2^64 is a bijection
SEED_LIMIT = 1 << 62                   # seeds live in [0, 2^62), as ResidualDiffusion._slice_seeds draws them


def splitmix64(z):
    """The finaliser of SplitMix64 (Steele, Lea, Flood 2014) on a Python int, mod 2^64."""
    z = (z + _GOLDEN) & _M64
    z = ((z ^ (z >> 30)) * _MUL1) & _M64
    z = ((z ^ (z >> 27)) * _MUL2) & _M64
    return z ^ (z >> 31)


def ensemble_seeds(slice_seeds, K):
    """(B, K) int64: replica 0 keeps the slice's seed s (a K = 1 ensemble is the sample of `slice_seeds`), replica k >= 1 gets
    splitmix64(s ^ (k * 0xD1B54A32D192ED03 mod 2^64)) >> 2."""
    K = int(K)
    if K < 1:
        raise RuntimeError(f"ensemble_seeds: K must be at least 1 (got {K})")
    seeds = [int(s) for s in np.asarray(slice_seeds).reshape(-1).tolist()]
    out = np.empty((len(seeds), K), dtype=np.int64)
    for b, s in enumerate(seeds):
        if not 0 <= s < SEED_LIMIT:
            raise RuntimeError(f"ensemble_seeds: seed {s} of slice {b} is outside [0, 2^62)")
        out[b, 0] = s
        for k in range(1, K):
            out[b, k] = splitmix64(s ^ ((k * _REPLICA) & _M64)) >> 2
    return out


def ensemble_passes(B, K, rows_max):
    """The B * K rows (slice-major: row b * K + k) as consecutive passes [(lo, hi), ...] of at most `rows_max` rows; every row once."""
    B, K, rows_max = int(B), int(K), int(rows_max)
    if B < 0 or K < 1 or rows_max < 1:
        raise RuntimeError(f"ensemble_passes: need B >= 0, K >= 1, rows_max >= 1 (got {B}, {K}, {rows_max})")
    R = B * K
    return [(lo, min(lo + rows_max, R)) for lo in range(0, R, rows_max)]
