"""Seeds, passes, quantile tables and orientation codes of an ensemble of K keyed realisations per slice
(ResidualDiffusion.sample_ensemble).  Pure numpy, no GPU.

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


QUANTILE_LEVELS_MAX = 8                # levels per call of fd_ensemble_order_f32


def quantile_table(levels, K):
    """(lo, hi int32, frac float32), one entry per level in the caller's order: level q of K sorted values v_(0) <= ... <= v_(K-1) is
    v_(lo) + frac (v_(hi) - v_(lo)), the `linear` rule of numpy.quantile / torch.quantile.  In float64 h = q (K - 1), an h within
    1e-9 of an integer is that integer (0.1 * 10 is not 1), lo = floor(h), hi = min(lo + 1, K - 1), frac = float32(h - lo).
    frac == 0 makes the level an exact selection: minimum, maximum, the median of an odd K, every level at K = 1."""
    K = int(K)
    if K < 1:
        raise RuntimeError(f"quantile_table: K must be at least 1 (got {K})")
    q = np.asarray(levels, dtype=np.float64).reshape(-1)
    if not 1 <= q.size <= QUANTILE_LEVELS_MAX:
        raise RuntimeError(f"quantile_table: 1 to {QUANTILE_LEVELS_MAX} levels per call (got {q.size})")
    if not np.isfinite(q).all() or q.min() < 0 or q.max() > 1:
        raise RuntimeError(f"quantile_table: levels must be finite and in [0, 1] (got {q.tolist()})")
    h = q * (K - 1)
    r = np.rint(h)
    h = np.where(np.abs(h - r) <= 1e-9, r, h)
    lo = np.floor(h)
    hi = np.minimum(lo + 1, K - 1)
    return lo.astype(np.int32), hi.astype(np.int32), (h - lo).astype(np.float32)


def quantile_suffix(levels):
    """['_q0050', ...]: a level's file-name suffix, the level in per-mille on four digits; levels that collide there raise"""
    names = ["_q%04d" % int(round(1000 * float(q))) for q in levels]
    if len(set(names)) != len(names):
        raise RuntimeError(f"quantile_suffix: levels {list(levels)} collide when rounded to per-mille ({names})")
    return names


# ---- orientation ensembles: replica k sees the slice under a flip / rot90 code and is turned back before the reduction
ORIENTATIONS_D4 = (0, 1, 2, 3, 4, 5, 6, 7)     # the 8 elements of the dihedral group of the square
ORIENTATIONS_FLIPS = (0, 1, 2, 3)              # the four that keep an H != W shape


def _orient(m, code):
    """diffusion_train.train_augment's code on a 2-D array: bit 0 flips H, bit 1 flips W, bits 2-3 are k"""
    if code & 1:
        m = m[::-1]
    if code & 2:
        m = m[:, ::-1]
    return np.rot90(m, (code >> 2) & 3)


def _inverse_table():
    g = np.arange(9).reshape(3, 3)             # 9 distinct values: no two elements of the group agree on it
    return tuple(next(c for c in range(8) if np.array_equal(_orient(_orient(g, code), c), g)) for code in range(16))


_INVERSE = _inverse_table()


def orientation_inverse(code):
    """The code c' in 0..7 whose map undoes `code` (0..15): augment_source_index(c') composed with augment_source_index(code) is
    the identity on a square.  Codes 8..15 reach the group's elements a second time and map to the inverse of theirs, so
    orientation_inverse(orientation_inverse(c)) is c's element as a code in 0..7."""
    if isinstance(code, bool) or not isinstance(code, (int, np.integer)) or not 0 <= int(code) <= 15:
        raise RuntimeError(f"orientation_inverse: a code is an integer in 0..15 (got {code!r})")
    return _INVERSE[int(code)]


def orientation_codes(orientations, K, square):
    """(K,) int32: replica k sees the slice under codes[k % len(codes)].  `orientations`: "d4" (ORIENTATIONS_D4; a square slice),
    "flips" (ORIENTATIONS_FLIPS) or a non-empty sequence of codes in 0..15.  K may be smaller or larger than the set: K = 16 with
    "d4" is every orientation under two noise seeds.  A transposing code (k odd) on a slice that is not square raises."""
    K = int(K)
    if K < 1:
        raise RuntimeError(f"orientation_codes: K must be at least 1 (got {K})")
    if isinstance(orientations, str):
        if orientations not in ("d4", "flips"):
            raise RuntimeError(f"orientation_codes: orientations must be 'd4', 'flips' or a sequence of codes (got {orientations!r})")
        if orientations == "d4" and not square:
            raise RuntimeError("orientation_codes: 'd4' turns the slice by 90 degrees and needs a square one: use 'flips'")
        codes = ORIENTATIONS_D4 if orientations == "d4" else ORIENTATIONS_FLIPS
    else:
        try:
            given = list(orientations)
        except TypeError:
            raise RuntimeError(f"orientation_codes: orientations must be 'd4', 'flips' or a sequence of codes (got {orientations!r})")
        if not given:
            raise RuntimeError("orientation_codes: an empty sequence of orientations")
        for c in given:
            if isinstance(c, (bool, str)) or not isinstance(c, (int, np.integer)) or not 0 <= int(c) <= 15:
                raise RuntimeError(f"orientation_codes: a code is an integer in 0..15 (got {c!r})")
        codes = tuple(int(c) for c in given)
        bad = [c for c in codes if c & 4]
        if bad and not square:
            raise RuntimeError(f"orientation_codes: codes {bad} transpose (k odd) and need a square slice")
    return np.asarray([codes[k % len(codes)] for k in range(K)], dtype=np.int32)


def ensemble_passes(B, K, rows_max):
    """The B * K rows (slice-major: row b * K + k) as consecutive passes [(lo, hi), ...] of at most `rows_max` rows; every row once."""
    B, K, rows_max = int(B), int(K), int(rows_max)
    if B < 0 or K < 1 or rows_max < 1:
        raise RuntimeError(f"ensemble_passes: need B >= 0, K >= 1, rows_max >= 1 (got {B}, {K}, {rows_max})")
    R = B * K
    return [(lo, min(lo + rows_max, R)) for lo in range(0, R, rows_max)]
