"""Seeds, passes, quantile tables and orientation codes of an ensemble of K keyed realisations per slice
(ResidualDiffusion.sample_ensemble).  Pure numpy, no GPU.

A replica is an ordinary slice of the samplers with a seed of its own: x_T and the ancestral sampler's step noise are functions of
(seed, step, pixel) alone (fd_keyed_normal), so replica k of a slice is the same image in any batch, on any rank and stream.
"""
import math
from fractions import Fraction
from typing import NamedTuple, Optional

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


# ---- calibrated intervals: one scale for both half-widths, chosen on held-out slices so that the share of missed pixels is controlled
class IntervalCalibration(NamedTuple):
    """risk_control's result.  scale = grid[g], g the smallest accepted index; risk = the empirical risk R(g) of the calibration
    slices at that scale, raw_risk = R at the largest grid value <= 1 (the unscaled interval; None if the grid has none);
    n_slices x n_pixels is what was counted; settings: what the scale is valid for (Trainer.calibrate_intervals fills it)."""
    scale: float
    g: int
    alpha: float
    bound: str
    delta: Optional[float]
    n_slices: int
    n_pixels: int
    risk: float
    raw_risk: Optional[float]
    grid_max: float
    settings: Optional[dict] = None


def interval_grid(max_scale=16.0, n=1025):
    """np.linspace(0, max_scale, n) as float32: the default grid of scales (an API default, not a tuned number)"""
    return np.linspace(0, max_scale, n).astype(np.float32)


def _exact(x):
    """the decimal the caller wrote (0.1 is 1/10, not the double next to it): acceptance is decided in rationals"""
    return Fraction(repr(float(x)))


def risk_control(hist, n_pixels, grid, alpha, bound="crc", delta=None):
    """The smallest scale of `grid` whose risk bound is at most `alpha`, from the counts of N calibration slices.
    hist (N, G + 1) integers: metrics.interval_hist's rows, hist[i][j] pixels of slice i in bin j, every row summing to n_pixels.
    cum[i][g] = hist[i][0] + ... + hist[i][g] pixels of slice i have a score <= grid[g]; the loss of slice i at g is
    1 - cum[i][g] / n_pixels and the empirical risk R(g) = (N n_pixels - sum_i cum[i][g]) / (N n_pixels), formed from Python
    integers and non-increasing in g.
    bound="crc" (conformal risk control, Angelopoulos et al. 2022): g is accepted iff (N R(g) + 1) / (N + 1) <= alpha, decided in
    rationals; the expected loss of a new slice exchangeable with the N is then at most alpha.  It needs 1 / (N + 1) <= alpha.
    bound="hoeffding" (needs 0 < delta < 1; Bates et al. 2021 with Hoeffding's inequality): g is accepted iff
    R(g) + sqrt(ln(1 / delta) / (2 N)) <= alpha; with probability at least 1 - delta over the calibration set the expected loss is at
    most alpha.  It needs N >= ln(1 / delta) / (2 alpha^2).
    Returns an IntervalCalibration; raises RuntimeError where no index is accepted, saying whether N is too small for the bound
    (and which N would do) or the grid ends too early (and R at its last value)."""
    g32 = np.asarray(grid, dtype=np.float32).reshape(-1)
    G = int(g32.size)
    h = np.asarray(hist)
    if h.ndim != 2 or h.shape[0] < 1 or h.shape[1] != G + 1 or not np.issubdtype(h.dtype, np.integer):
        raise RuntimeError(f"risk_control: hist must be an (N, G + 1) = (N, {G + 1}) integer array with N >= 1 (got shape "
                           f"{tuple(h.shape)}, dtype {h.dtype})")
    N, n_pixels = int(h.shape[0]), int(n_pixels)
    rows = [[int(v) for v in r] for r in h.tolist()]
    if n_pixels < 1 or any(min(r) < 0 or sum(r) != n_pixels for r in rows):
        raise RuntimeError(f"risk_control: every row of hist must be non-negative and sum to n_pixels = {n_pixels}")
    if bound not in ("crc", "hoeffding"):
        raise RuntimeError(f"risk_control: bound must be 'crc' or 'hoeffding' (got {bound!r})")
    if not 0 < float(alpha) < 1:
        raise RuntimeError(f"risk_control: alpha must be in (0, 1) (got {alpha})")
    if bound == "hoeffding":
        if delta is None or not 0 < float(delta) < 1:
            raise RuntimeError(f"risk_control: bound='hoeffding' needs 0 < delta < 1 (got {delta})")
        delta = float(delta)
    elif delta is not None:
        raise RuntimeError("risk_control: delta belongs to bound='hoeffding' (bound='crc' takes none)")
    alpha = float(alpha)
    total = N * n_pixels
    miss, covered = [], 0                                                # miss[g] = N n_pixels - sum_i cum[i][g]
    for g in range(G):
        covered += sum(r[g] for r in rows)
        miss.append(total - covered)
    if bound == "crc":
        a = _exact(alpha)
        ok = lambda g: Fraction(miss[g] + n_pixels, n_pixels * (N + 1)) <= a
        feasible = Fraction(1, N + 1) <= a
        need = int(math.ceil(1 / a - 1))
        limit = f"conformal risk control needs 1 / (N + 1) <= alpha: N >= {need} calibration slices at alpha = {alpha}"
    else:
        slack = math.sqrt(math.log(1 / delta) / (2 * N))
        ok = lambda g: miss[g] / total + slack <= alpha
        feasible = slack <= alpha
        need = int(math.ceil(math.log(1 / delta) / (2 * alpha * alpha)))
        limit = (f"the Hoeffding bound needs N >= ln(1 / delta) / (2 alpha^2): N >= {need} calibration slices at alpha = {alpha}, "
                 f"delta = {delta}")
    star = next((g for g in range(G) if ok(g)), None)
    if star is None:
        if not feasible:
            raise RuntimeError(f"risk_control: N = {N} is too small for the bound: {limit}")
        raise RuntimeError(f"risk_control: the grid ends too early: at its last value {float(g32[-1])} the empirical risk "
                           f"R({G - 1}) = {miss[-1] / total} is still not accepted at alpha = {alpha}: extend the grid")
    raw = [g for g in range(G) if g32[g] <= 1]
    return IntervalCalibration(scale=float(g32[star]), g=star, alpha=alpha, bound=bound, delta=delta, n_slices=N, n_pixels=n_pixels,
                               risk=miss[star] / total, raw_risk=miss[raw[-1]] / total if raw else None, grid_max=float(g32[-1]))


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
