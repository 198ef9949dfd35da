"""founddiff_amd/tiling.py without a GPU: the plan of overlapping tiles along an axis, their blend weights, the tiles' seeds and the
cut of the tile rows into passes, against the formulas written out here."""
import numpy as np
import pytest

from founddiff_amd.ensemble import ensemble_seeds
from founddiff_amd.tiling import tile_pair, tile_passes, tile_plan, tile_seeds, tile_weights


def _cover(origins, n, tile):
    c = np.zeros(n, dtype=np.int64)
    for a in origins:
        c[a:a + tile] += 1
    return c


def blend64(tiles, ys, xs, wy, wx, H, W):
    """the float64 blend of tiles [my][mx][th][tw]: sum w v / sum w, w = wy[iy][:, None] wx[ix][None, :]"""
    th, tw = tiles.shape[-2:]
    num, den = np.zeros((H, W)), np.zeros((H, W))
    for iy, ya in enumerate(ys):
        for ix, xa in enumerate(xs):
            w = wy[iy].astype(np.float64)[:, None] * wx[ix].astype(np.float64)[None, :]
            num[ya:ya + th, xa:xa + tw] += w * tiles[iy, ix]
            den[ya:ya + th, xa:xa + tw] += w
    return num / den


@pytest.mark.parametrize("tile", [8, 16, 32])
def test_tile_plan_every_legal_case(tile):
    for n in range(max(8, tile), 81):
        for overlap in range(0, tile // 2 + 1):
            a = tile_plan(n, tile, overlap)
            s = tile - overlap
            m = 1 if n == tile else -(-(n - tile) // s) + 1
            assert a.dtype.kind == "i" and len(a) == m, (n, tile, overlap)
            assert a[0] == 0 and a[-1] == n - tile
            assert (np.diff(a) > 0).all()
            assert all(a[i] == min(i * s, n - tile) for i in range(m))
            assert all(a[i] + tile - a[i + 1] >= overlap for i in range(m - 1))
            assert (_cover(a, n, tile) >= 1).all()


def test_shifted_last_tile():
    a = tile_plan(22, 8, 4)
    assert a.tolist() == [0, 4, 8, 12, 14]
    c = _cover(a, 22, 8)
    assert c[14] == 3 and c[15] == 3 and c.max() == 3
    w = tile_weights(a, 22, 8)
    # the last tile ramps over its real overlap with its neighbour, 12 + 8 - 14 = 6 pixels
    assert np.array_equal(w[4], np.minimum(1, (np.arange(8) + 1) / 7).astype(np.float32))


@pytest.mark.parametrize("n,tile,overlap", [(8, 8, 0), (22, 8, 4), (27, 8, 4), (64, 32, 8), (80, 16, 8), (33, 32, 16), (64, 16, 0)])
def test_tile_weights(n, tile, overlap):
    a = tile_plan(n, tile, overlap)
    w = tile_weights(a, n, tile)
    m = len(a)
    assert w.shape == (m, tile) and w.dtype == np.float32
    assert (w > 0).all() and (w <= 1).all()
    if overlap == 0 and (n - tile) % tile == 0:
        assert (w == 1).all()
    # a side on the border of the image does not ramp: the first tile's left part and the last tile's right part
    r_hi0 = a[0] + tile - a[1] if m > 1 else 0
    r_lo_last = a[-2] + tile - a[-1] if m > 1 else 0
    assert (w[0, :tile - r_hi0] == 1).all() and (w[-1, r_lo_last:] == 1).all()
    # exactly 1 wherever one tile alone covers a pixel
    c = _cover(a, n, tile)
    for i in range(m):
        assert (w[i][c[a[i]:a[i] + tile] == 1] == 1).all()
    # the formula, tile by tile
    u = np.arange(tile, dtype=np.float64)
    for i in range(m):
        wl = np.ones(tile) if i == 0 else np.minimum(1, (u + 1) / (a[i - 1] + tile - a[i] + 1))
        wh = np.ones(tile) if i == m - 1 else np.minimum(1, (tile - u) / (a[i] + tile - a[i + 1] + 1))
        assert np.array_equal(w[i], np.minimum(wl, wh).astype(np.float32))


def test_overlap_zero_is_weight_one():
    for tile in (8, 16, 32):
        for n in range(tile, 161, tile):
            assert (tile_weights(tile_plan(n, tile, 0), n, tile) == 1).all()
    # (a last tile that is shifted back overlaps its neighbour whatever `overlap` says, and the two ramp there)
    w = tile_weights(tile_plan(70, 16, 0), 70, 16)
    assert (w[:3] == 1).all() and (w[3:] < 1).any() and (w > 0).all()


@pytest.mark.parametrize("H,W,th,tw,oy,ox", [(8, 8, 8, 8, 0, 0), (22, 27, 8, 8, 4, 4), (64, 64, 32, 32, 8, 8), (40, 70, 16, 32, 3, 16)])
def test_float64_blend_returns_the_image(H, W, th, tw, oy, ox):
    img = np.random.default_rng(H * W).random((H, W))
    ys, xs = tile_plan(H, th, oy), tile_plan(W, tw, ox)
    wy, wx = tile_weights(ys, H, th), tile_weights(xs, W, tw)
    tiles = np.stack([np.stack([img[y:y + th, x:x + tw] for x in xs]) for y in ys])
    assert float(np.abs(blend64(tiles, ys, xs, wy, wx, H, W) - img).max()) <= 1e-12


def test_tile_seeds():
    seeds = np.arange(4096, dtype=np.int64)
    t = tile_seeds(seeds, 16)
    assert t.shape == (4096, 16) and t.dtype == np.int64
    assert np.array_equal(t[:, 0], seeds)
    assert int(t.min()) >= 0 and int(t.max()) < 2 ** 62
    assert len(np.unique(t)) == t.size
    e = ensemble_seeds(seeds, 16)
    assert not (t[:, 1:] == e[:, 1:]).any()
    big = tile_seeds([2 ** 62 - 1, 2 ** 40 + 5], 3)
    assert big[0, 0] == 2 ** 62 - 1 and int(big.min()) >= 0 and int(big.max()) < 2 ** 62
    assert np.array_equal(tile_seeds([7], 1), [[7]])


def test_tile_passes():
    for B, my, mx, rows_max in ((3, 3, 3, 4), (1, 1, 1, 32), (2, 5, 4, 32), (0, 2, 2, 8), (4, 2, 3, 24)):
        p = tile_passes(B, my, mx, rows_max)
        R = B * my * mx
        assert all(0 < hi - lo <= rows_max for lo, hi in p)
        assert [r for lo, hi in p for r in range(lo, hi)] == list(range(R))
    assert tile_passes(3, 3, 3, 4) == [(0, 4), (4, 8), (8, 12), (12, 16), (16, 20), (20, 24), (24, 27)]
    # the fewest passes, then of equal size: one loop graph serves them all
    assert tile_passes(8, 3, 3, 32) == [(0, 24), (24, 48), (48, 72)]
    assert tile_passes(5, 3, 3, 32) == [(0, 23), (23, 45)] and tile_passes(5, 3, 3, 32, 2) == [(0, 24), (24, 45)]
    assert tile_passes(1, 3, 3, 32, 2) == [(0, 9)] and tile_passes(2, 3, 3, 4, 2) == [(0, 4), (4, 8), (8, 12), (12, 16), (16, 18)]
    with pytest.raises(RuntimeError, match="multiple of multiple"):
        tile_passes(1, 3, 3, 5, 2)


def test_errors():
    with pytest.raises(RuntimeError, match="1 <= tile <= n .got tile 9, n 8"):
        tile_plan(8, 9, 0)
    with pytest.raises(RuntimeError, match="1 <= tile <= n .got tile 0, n 8"):
        tile_plan(8, 0, 0)
    with pytest.raises(RuntimeError, match="0 <= overlap <= tile // 2 .got overlap 5, tile 8"):
        tile_plan(16, 8, 5)
    with pytest.raises(RuntimeError, match="0 <= overlap <= tile // 2 .got overlap -1, tile 8"):
        tile_plan(16, 8, -1)
    with pytest.raises(RuntimeError, match="do not cover an axis of length 22"):
        tile_weights([0, 4, 8], 22, 8)
    with pytest.raises(RuntimeError, match="n_tiles must be at least 1"):
        tile_seeds([1], 0)
    with pytest.raises(RuntimeError, match="outside"):
        tile_seeds([2 ** 62], 2)
    with pytest.raises(RuntimeError, match="outside"):
        tile_seeds([-1], 2)
    with pytest.raises(RuntimeError, match="my, mx >= 1"):
        tile_passes(1, 0, 1, 4)
    with pytest.raises(RuntimeError, match="rows_max >= 1"):
        tile_passes(1, 1, 1, 0)
    with pytest.raises(RuntimeError, match="tile must be an int or a pair"):
        tile_pair("f", 2.5, "tile")
    assert tile_pair("f", 3, "tile") == (3, 3) and tile_pair("f", (3, 4), "tile") == (3, 4)


def test_public_interface_exists():
    """sample_tiled and its callers' arguments: signatures only, nothing runs"""
    import inspect
    from founddiff_amd import _lib, parallel
    from founddiff_amd.DADiff import ResidualDiffusion, Trainer
    sig = inspect.signature(ResidualDiffusion.sample_tiled)
    assert list(sig.parameters) == ["self", "x_input", "tile", "overlap", "slice_seeds", "condition"]
    assert sig.parameters["overlap"].default == 0 and sig.parameters["condition"].default == "tile"
    p = inspect.signature(Trainer.test).parameters
    assert p["tile"].default is None and p["overlap"].default == 0 and p["tile_condition"].default == "tile"
    assert inspect.signature(Trainer.__init__).parameters["val_crop_size"].default is None
    p = inspect.signature(parallel.sample_volume).parameters
    assert p["tile"].default is None and p["overlap"].default == 0
    assert "fd_tiles_gather_f32" in _lib.SIGNATURES and "fd_tiles_blend_f32" in _lib.SIGNATURES
