"""The numpy oracle of the calibrated intervals (fd_interval_hist_f32, fd_interval_scale_f32, ensemble.risk_control) and the cases
the CPU and the GPU tests share.  Everything here is float32 numpy, one rounding per written operation, which is what the kernels
are held to bit for bit; risk_control is redone in rationals."""
from fractions import Fraction
import math

import numpy as np

FLOOR = np.float32(1 / 3000)
F32 = np.float32

# grids of exact dyadic values, so that a planted score can equal a grid value bit for bit: G = 1, 2, 33, 4096
GRIDS = {
    1: np.array([1.0], np.float32),
    2: np.array([0.5, 2.0], np.float32),
    33: np.linspace(0, 16, 33).astype(np.float32),                       # steps of 1/2
    4096: (np.arange(4096) / 256).astype(np.float32),                    # steps of 2^-8, up to 16 - 2^-8
}


def half_widths(m, l, u, floor=FLOOR):
    with np.errstate(invalid="ignore"):
        return np.fmax((m - l).astype(F32), F32(floor)), np.fmax((u - m).astype(F32), F32(floor))


def score(m, l, u, y, floor=FLOOR):
    """(s, out): the score of every pixel in float32 and whether no scale covers it for want of a number"""
    m, l, u, y = (np.asarray(v, F32) for v in (m, l, u, y))
    d_lo, d_hi = half_widths(m, l, u, floor)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        a = ((m - y).astype(F32) / d_lo).astype(F32)
        b = ((y - m).astype(F32) / d_hi).astype(F32)
    out = np.isnan(m) | np.isnan(l) | np.isnan(u) | np.isnan(y) | np.isnan(a) | np.isnan(b)
    return np.fmax(a, b), out


def bins(s, out, grid):
    """the number of grid values strictly below s; G where `out`"""
    grid = np.asarray(grid, F32)
    b = np.searchsorted(grid, np.where(out, F32(np.inf), s), side="left")
    return np.where(out, grid.size, b)


def hist(m, l, u, y, grid, floor=FLOOR):
    """(B, G + 1) int64 from maps (B, n)"""
    G = np.asarray(grid).size
    s, out = score(m, l, u, y, floor)
    b = bins(s, out, grid)
    return np.stack([np.bincount(row, minlength=G + 1) for row in b.reshape(b.shape[0], -1)]).astype(np.int64)


def scale_maps(m, l, u, scale, floor=FLOOR):
    """(lo_out, hi_out) float32: the product and the sum two roundings, clamped to [0, 1]; NaN where m, l or u is"""
    m, l, u = (np.asarray(v, F32) for v in (m, l, u))
    d_lo, d_hi = half_widths(m, l, u, floor)
    with np.errstate(invalid="ignore", over="ignore"):
        lo = (m - (F32(scale) * d_lo).astype(F32)).astype(F32)
        hi = (m + (F32(scale) * d_hi).astype(F32)).astype(F32)
        lo, hi = np.minimum(np.maximum(lo, F32(0)), F32(1)), np.minimum(np.maximum(hi, F32(0)), F32(1))
    nan = np.isnan(m) | np.isnan(l) | np.isnan(u)
    return np.where(nan, F32(np.nan), lo).astype(F32), np.where(nan, F32(np.nan), hi).astype(F32)


def risk(counts, n_pixels, g):
    """R(g) as a Fraction"""
    counts = [[int(v) for v in r] for r in np.asarray(counts).tolist()]
    N = len(counts)
    covered = sum(sum(r[:g + 1]) for r in counts)
    return Fraction(N * n_pixels - covered, N * n_pixels)


def risk_control(counts, n_pixels, grid, alpha, bound="crc", delta=None):
    """(g*, scale, R(g*)) by the definitions, in rationals (the Hoeffding slack in float64); None where nothing is accepted"""
    N, G = len(counts), len(grid)
    a = Fraction(repr(float(alpha)))
    for g in range(G):
        R = risk(counts, n_pixels, g)
        if bound == "crc":
            ok = (N * R + 1) / (N + 1) <= a
        else:
            ok = float(R) + math.sqrt(math.log(1 / delta) / (2 * N)) <= alpha
        if ok:
            return g, float(np.asarray(grid, F32)[g]), R
    return None


def planted_maps(B, n, grid, seed):
    """(m, l, u, y) float32 (B, n): random maps with, where n leaves room, pixels whose score equals a grid value exactly on the
    lower and on the upper side (m = 1/2, d_lo = 1/8, d_hi = 1/4 and a dyadic grid: every operation exact), l = m = u (the floor),
    y == m, m outside [l, u], and y = +-inf.  NaNs are planted by the caller."""
    rng = np.random.default_rng(seed)
    grid = np.asarray(grid, F32)
    m = rng.random((B, n), dtype=F32)
    l = (m - F32(0.1) * rng.random((B, n), dtype=F32)).astype(F32)
    u = (m + F32(0.1) * rng.random((B, n), dtype=F32)).astype(F32)
    y = (m + F32(0.15) * rng.standard_normal((B, n), dtype=F32)).astype(F32)
    spots = iter(rng.permutation(n).tolist())

    def put(b, vm, vl, vu, vy):
        i = next(spots, None)
        if i is not None:
            m[b, i], l[b, i], u[b, i], y[b, i] = vm, vl, vu, vy
    for b in range(B):
        for g in sorted({0, grid.size // 2, grid.size - 1}):
            put(b, 0.5, 0.375, 0.75, F32(0.5) - grid[g] * F32(0.125))    # s == grid[g] from below the centre
            put(b, 0.5, 0.375, 0.75, F32(0.5) + grid[g] * F32(0.25))     # ... and from above
        put(b, 0.25, 0.25, 0.25, 0.2501)                                 # all replicas agree: both half-widths are the floor
        put(b, 0.5, 0.4, 0.6, 0.5)                                       # y == m: s = 0
        put(b, 0.7, 0.3, 0.6, 0.65)                                      # the mean above the upper level
        put(b, 0.2, 0.3, 0.6, 0.1)                                       # ... and below the lower one
        put(b, 0.5, 0.4, 0.6, np.inf)
        put(b, 0.5, 0.4, 0.6, -np.inf)
    return m, l, u, y


def toy_slices(rng, N, size=64, K=8):
    """The toy model of exchangeable draws: per pixel K clamped normal draws and one more as the truth, around a mean in tissue
    with a per-pixel sigma; the left third of every slice is air, where everything clamps to 0.  -> (mean, q05, q95, truth), each
    (N, size * size) float32, the levels by numpy's linear rule."""
    mu = rng.uniform(0.2, 0.8, (N, size, size))
    sigma = rng.uniform(0.005, 0.03, (N, size, size))
    draws = mu[:, None] + sigma[:, None] * rng.standard_normal((N, K + 1, size, size))
    draws[..., : size // 3] = -1.0                                       # air: far below the window
    draws = np.clip(draws, 0, 1).astype(F32)
    ens, truth = draws[:, :K], draws[:, K]
    q = np.quantile(ens, (0.05, 0.95), axis=1).astype(F32)
    flat = lambda a: a.reshape(N, -1)
    return flat(ens.mean(1, dtype=F32)), flat(q[0]), flat(q[1]), flat(truth)
