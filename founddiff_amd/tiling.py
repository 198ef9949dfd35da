"""Geometry, weights, seeds and passes of a slice sampled as overlapping tiles (ResidualDiffusion.sample_tiled).  Pure numpy, no GPU.

A tile is an ordinary slice of the samplers, th x tw pixels cut from the (H, W) slice, with a seed of its own; the tiles' final images
are blended back with separable ramp weights (csrc/fd_tiles.hip).  Along one axis of length n the tiles start every tile - overlap
pixels and the last one is shifted back to end at the border, so it may overlap its neighbour by more than `overlap`.
"""
import numpy as np

from .ensemble import SEED_LIMIT, _M64, ensemble_passes, ensemble_seeds, splitmix64

_TILE = 0xA0761D6478BD642F             # odd, and not ensemble._REPLICA: tile j and replica j of a slice get different streams


def tile_pair(fn, v, name):
    """`v` as (vy, vx): an int, or a pair of integers"""
    is_int = lambda a: isinstance(a, (int, np.integer)) and not isinstance(a, (bool, np.bool_))
    p = (v, v) if is_int(v) else v
    if not (isinstance(p, (tuple, list)) and len(p) == 2 and all(is_int(a) for a in p)):
        raise RuntimeError(f"{fn}: {name} must be an int or a pair of integers (got {v!r})")
    return int(p[0]), int(p[1])


def tile_plan(n, tile, overlap):
    """The origins of the tiles along an axis of length n, an int64 array: stride s = tile - overlap, m = 1 tiles if n == tile, else
    ceil((n - tile) / s) + 1, origin a_i = min(i s, n - tile).  1 <= tile <= n and 0 <= overlap <= tile // 2."""
    n, tile, overlap = int(n), int(tile), int(overlap)
    if not 1 <= tile <= n:
        raise RuntimeError(f"tile_plan: need 1 <= tile <= n (got tile {tile}, n {n})")
    if not 0 <= overlap <= tile // 2:
        raise RuntimeError(f"tile_plan: need 0 <= overlap <= tile // 2 (got overlap {overlap}, tile {tile})")
    s = tile - overlap
    m = 1 if n == tile else -((tile - n) // s) + 1
    return np.minimum(np.arange(m, dtype=np.int64) * s, n - tile)


def tile_weights(origins, n, tile):
    """(m, tile) float32: the weight of tile i at its local coordinate u.  Towards a neighbour the weight ramps over the REAL overlap
    with it, r_lo = a_{i-1} + tile - a_i and r_hi = a_i + tile - a_{i+1}: wl = min(1, (u + 1) / (r_lo + 1)), wh = min(1, (tile - u) /
    (r_hi + 1)), w = min(wl, wh); a side on the border of the image does not ramp (wl = 1 for i = 0, wh = 1 for i = m - 1).  Every
    weight is positive, and exactly 1 where nothing overlaps.  The 2-D weight of a tile is wy[iy][:, None] * wx[ix][None, :]."""
    a = np.asarray(origins, dtype=np.int64).reshape(-1)
    n, tile, m = int(n), int(tile), a.shape[0]
    if m < 1 or a[0] != 0 or a[-1] != n - tile or (m > 1 and (np.diff(a) <= 0).any()) or (m > 1 and (np.diff(a) > tile).any()):
        raise RuntimeError(f"tile_weights: origins {a.tolist()} do not cover an axis of length {n} with tiles of {tile}")
    u = np.arange(tile, dtype=np.float64)
    w = np.ones((m, tile), dtype=np.float64)
    for i in range(m):
        if i > 0:
            r_lo = a[i - 1] + tile - a[i]
            w[i] = np.minimum(w[i], np.minimum(1.0, (u + 1) / (r_lo + 1)))
        if i < m - 1:
            r_hi = a[i] + tile - a[i + 1]
            w[i] = np.minimum(w[i], np.minimum(1.0, (tile - u) / (r_hi + 1)))
    return w.astype(np.float32)


def tile_owner(ys, xs, H, W, th, tw):
    """(H, W) int64: per pixel the first tile that covers it in row-major tile order, iy * len(xs) + ix with iy ascending, then ix
    (-1 where none does) -- the tile whose lane writes the slice pixel in csrc/fd_tiles_step.hip."""
    ys, xs = np.asarray(ys, dtype=np.int64).reshape(-1), np.asarray(xs, dtype=np.int64).reshape(-1)
    owner = np.full((int(H), int(W)), -1, dtype=np.int64)
    for iy in range(len(ys) - 1, -1, -1):                      # descending, so that the first cover is written last
        for ix in range(len(xs) - 1, -1, -1):
            owner[ys[iy]:ys[iy] + th, xs[ix]:xs[ix] + tw] = iy * len(xs) + ix
    return owner


def tile_seeds(slice_seeds, n_tiles):
    """(B, n_tiles) int64: tile 0 keeps the slice's seed s (a one-tile plan is the sample of `slice_seeds`), tile j >= 1 gets
    splitmix64(s ^ (j * 0xA0761D6478BD642F mod 2^64)) >> 2."""
    n_tiles = int(n_tiles)
    if n_tiles < 1:
        raise RuntimeError(f"tile_seeds: n_tiles must be at least 1 (got {n_tiles})")
    seeds = [int(s) for s in np.asarray(slice_seeds).reshape(-1).tolist()]
    out = np.empty((len(seeds), n_tiles), dtype=np.int64)
    for b, s in enumerate(seeds):
        if not 0 <= s < SEED_LIMIT:
            raise RuntimeError(f"tile_seeds: seed {s} of slice {b} is outside [0, 2^62)")
        out[b, 0] = s
        for j in range(1, n_tiles):
            out[b, j] = splitmix64(s ^ ((j * _TILE) & _M64)) >> 2
    return out


def tiled_ensemble_seeds(slice_seeds, K, n_tiles):
    """(B, K, n_tiles) int64, the seeds of a tiled ensemble (ResidualDiffusion.sample_ensemble(tile=...)): replica first, then tile,
    tile_seeds(ensemble_seeds(slice_seeds, K).reshape(-1), n_tiles).  [b, 0, 0] is the slice's own seed and [:, k, :] is tile_seeds
    of replica k's seed, so a replica is an ordinary sample_tiled call under its ensemble seed.  The rows lie slice-major, then
    replica, then tile: row ((b K + k) my + iy) mx + ix."""
    K, n_tiles = int(K), int(n_tiles)
    if K < 1:
        raise RuntimeError(f"tiled_ensemble_seeds: K must be at least 1 (got {K})")
    if n_tiles < 1:
        raise RuntimeError(f"tiled_ensemble_seeds: n_tiles must be at least 1 (got {n_tiles})")
    seeds = [int(s) for s in np.asarray(slice_seeds).reshape(-1).tolist()]
    for b, s in enumerate(seeds):
        if not 0 <= s < SEED_LIMIT:
            raise RuntimeError(f"tiled_ensemble_seeds: seed {s} of slice {b} is outside [0, 2^62)")
    return tile_seeds(ensemble_seeds(seeds, K).reshape(-1), n_tiles).reshape(len(seeds), K, n_tiles)


def tiled_ensemble_opt_in(fn, tile, n_samples, tiled_ensemble):
    """The callers of the samplers (`fn`: Trainer.test, sample_volume) run an ensemble of tiled samples only on request: `tile`
    with n_samples > 1 raises without `tiled_ensemble` (the raising default is pinned by tests)."""
    if tile is not None and int(n_samples) > 1 and not tiled_ensemble:
        raise RuntimeError(f"{fn}: tile={tile!r} with n_samples={n_samples}: ensembles of tiled samples are opt-in: pass "
                           "tiled_ensemble=True (DESIGN.md section 8)")


def tile_passes(B, my, mx, rows_max, multiple=1):
    """The B * my * mx tile rows (slice-major: row (b * my + iy) * mx + ix) as consecutive passes [(lo, hi), ...] of at most
    `rows_max` rows; every row once.  ensemble_passes, asked for the fewest passes that `rows_max` allows and then for passes of
    equal size (72 rows at 32: three passes of 24, not 32 + 32 + 8): an engine keeps one captured loop graph per batch size, so
    passes of one size are captured once and ragged ones at every change of size.  `multiple` (a divisor of rows_max: the
    sampler's streams) rounds the size up, so that a pass still splits over the streams."""
    B, my, mx, rows_max, multiple = int(B), int(my), int(mx), int(rows_max), int(multiple)
    if my < 1 or mx < 1:
        raise RuntimeError(f"tile_passes: need my, mx >= 1 (got {my}, {mx})")
    if B < 0 or rows_max < 1:
        raise RuntimeError(f"tile_passes: need B >= 0, rows_max >= 1 (got {B}, {rows_max})")
    if multiple < 1 or rows_max % multiple:
        raise RuntimeError(f"tile_passes: rows_max must be a multiple of multiple >= 1 (got {rows_max}, {multiple})")
    R = B * my * mx
    n = max(1, -(-R // rows_max))
    size = max(1, -(-R // n))
    return ensemble_passes(B, my * mx, -(-size // multiple) * multiple)
