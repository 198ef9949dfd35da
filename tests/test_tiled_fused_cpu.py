"""Per-step fused tiled sampling without a GPU: a float64 numpy reference of one fused step (csrc/fd_tiles_step.hip: blend the tiles'
raw model outputs per pixel with blend64's rule, then the update of modes 0-3 in the DDIM and in the keyed ancestral form), checked
against itself -- a one-tile plan is the plain update, rows cut from slice-level tensors give the slice-level update on every tile,
common pixels of overlapping tiles come out identical, a tile pixel's noise is the slice's -- and tiling.tile_owner, the entry
points' argument checks and the host-side arguments of sample_tiled(fuse=).  tests/test_gpu_tiled_fused.py imports the reference.

step64's bound is test_gpu_obj_loop._ref64's (first order in u = 2^-24, every fp32 operation u |its result|), with errors e0 / e1 of
the inputs o0 / o1 carried through the formulas: clamp is 1-Lipschitz, a product by a constant scales an error by |constant|, a sum
adds them.  fused_step64 feeds it the blend's (2 c + 4) u max|v| per blended stream (tests/test_gpu_tiled.py's docstring)."""
import os
import sys

import numpy as np
import pytest

from test_tiling_cpu import blend64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
PLANS = [(8, 8, 8, 8, 0), (22, 27, 8, 8, 4), (64, 64, 32, 32, 8)]          # (H, W, th, tw, overlap): tests/test_gpu_tiled.py CASES


def step64(mode, form, o0, o1, x, xi, row, z=None, t=0, e0=0.0, e1=0.0):
    """(value, first-order rounding bound) in float64 of one pixel update.  form "keyed": row = {ac, bc, omac, c1, c2, c3, logvar,
    -}, out = c1 x + c2 pred_res + c3 x_start + exp(logvar / 2) z, no noise at t = 0; "ddim": row = {ac, bc, omac, alpha, -, -, -,
    last}, out = x_start if last else x - alpha pred_res.  e0 / e1: what o0 / o1 may already be off by."""
    a, bb, oma = [float(v) for v in row[:3]]
    clamp = lambda v: np.clip(v, -1.0, 1.0)
    zero = np.zeros_like(x)
    if mode == 0:
        pr, e_pr = clamp(o0), e0 + zero
        d = xi - pr
        xs, e_xs = clamp(d), e_pr + U * np.abs(d)
    elif mode in (1, 2):
        y, e_y = (xi, zero) if mode == 1 else (clamp(o0), e0 + zero)
        p1 = a * y
        r1 = x - p1
        p2 = bb * o1
        n = r1 - p2
        e_n = U * (np.abs(p1) + np.abs(r1) + np.abs(p2) + np.abs(n)) + abs(a) * e_y + abs(bb) * e1
        if mode == 1:
            q = n / oma
            xs, e_xs = clamp(q), e_n / abs(oma) + U * np.abs(q)
            d = xi - xs
            pr, e_pr = clamp(d), e_xs + U * np.abs(d)
        else:
            pr, e_pr, xs, e_xs = y, e_y, clamp(n), e_n
    else:
        d = xi - o0
        pr, e_pr = clamp(d), e0 + U * np.abs(d)
        xs, e_xs = clamp(o0), e0 + zero
    if form == "ddim":
        alpha, last = float(row[3]), float(row[7]) != 0.0
        if last:
            return xs, e_xs * (1 + 2.0 ** -10)
        v = x - alpha * pr
        return v, (abs(alpha) * e_pr + U * (np.abs(alpha * pr) + np.abs(v))) * (1 + 2.0 ** -10)
    c1, c2, c3, lv = [float(v) for v in row[3:7]]
    sd = float(np.exp(0.5 * lv)) if t > 0 else 0.0
    terms = [c1 * x, c2 * pr, c3 * xs, sd * (zero if z is None else z)]
    mag = sum(np.abs(v) for v in terms)
    bound = abs(c2) * e_pr + abs(c3) * e_xs + U * mag + 4 * U * np.abs(terms[3]) + 3 * U * mag
    return sum(terms), bound * (1 + 2.0 ** -10)


def cut(img, ys, xs, th, tw):
    """[my][mx][th][tw]: the windows of img [H][W] by numpy indexing"""
    return np.stack([np.stack([img[y:y + th, x:x + tw] for x in xs]) for y in ys])


def fused_step64(mode, form, o0, o1, x_t, x_in, row, ys, xs, wy, wx, H, W, z=None, t=0):
    """One fused step of one slice in float64.  o0, o1, x_t, x_in: [my][mx][th][tw] tile rows (o0 / o1 None where the mode does not
    read it), z: the SLICE's noise [H][W].  Returns (rows [my][mx][th][tw], bound of the same shape, slice [H][W] assembled from
    every pixel's first covering tile)."""
    from founddiff_amd.tiling import tile_owner
    th, tw = x_t.shape[-2:]
    c = np.zeros((H, W))
    for ya in ys:
        for xa in xs:
            c[ya:ya + th, xa:xa + tw] += 1

    def blended(o):
        if o is None:
            return None, 0.0
        vmax = np.zeros((H, W))
        for iy, ya in enumerate(ys):
            for ix, xa in enumerate(xs):
                win = (slice(ya, ya + th), slice(xa, xa + tw))
                vmax[win] = np.maximum(vmax[win], np.abs(o[iy, ix]))
        return cut(blend64(o, ys, xs, wy, wx, H, W), ys, xs, th, tw), cut((2 * c + 4) * U * vmax, ys, xs, th, tw)
    b0, e0 = blended(o0 if mode != 1 else None)
    b1, e1 = blended(o1 if mode in (1, 2) else None)
    zr = None if z is None else cut(z, ys, xs, th, tw)
    rows, bound = step64(mode, form, b0, b1, x_t, x_in, row, zr, t, e0, e1)
    owner = tile_owner(ys, xs, H, W, th, tw)
    out = np.zeros((H, W))
    for iy, ya in enumerate(ys):
        for ix, xa in enumerate(xs):
            m = owner[ya:ya + th, xa:xa + tw] == iy * len(xs) + ix
            out[ya:ya + th, xa:xa + tw][m] = rows[iy, ix][m]
    return rows, bound, out


def _geometry(H, W, th, tw, overlap):
    from founddiff_amd.tiling import tile_plan, tile_weights
    ys, xs = tile_plan(H, th, overlap), tile_plan(W, tw, overlap)
    return ys, xs, tile_weights(ys, H, th), tile_weights(xs, W, tw)


def _rows(seed):
    """keyed row {ac, bc, omac, c1, c2, c3, logvar, 0} and DDIM rows {ac, bc, omac, alpha, 0, 0, 0, last}"""
    g = np.random.default_rng(seed)
    ac, bc = g.uniform(0.1, 0.9), g.uniform(0.01, 0.1)
    keyed = np.array([ac, bc, 1 - ac, 0.7, 0.2, 0.1, -6.0, 0.0])
    return keyed, np.array([ac, bc, 1 - ac, 0.05, 0, 0, 0, 0.0]), np.array([ac, bc, 1 - ac, 0.0, 0, 0, 0, 1.0])


def _forms(seed):
    keyed, ddim, ddim_last = _rows(seed)
    return [("keyed", keyed, 17), ("keyed", keyed, 0), ("ddim", ddim, 0), ("ddim", ddim_last, 0)]


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_one_tile_plan_is_the_plain_update(mode):
    H = W = 8
    ys, xs, wy, wx = _geometry(H, W, 8, 8, 0)
    g = np.random.default_rng(mode)
    o0, o1, x, xi, z = (g.standard_normal((1, 1, H, W)) for _ in range(5))
    for form, row, t in _forms(mode):
        rows, bound, out = fused_step64(mode, form, o0, o1, x, xi, row, ys, xs, wy, wx, H, W, z[0, 0], t)
        want, _ = step64(mode, form, o0, o1, x, xi, row, z, t)
        assert np.array_equal(rows, want) and np.array_equal(out, want[0, 0]) and bound.shape == rows.shape
    # no noise at t = 0, noise at t > 0
    keyed = _rows(mode)[0]
    a = fused_step64(mode, "keyed", o0, o1, x, xi, keyed, ys, xs, wy, wx, H, W, z[0, 0], 0)[0]
    b = fused_step64(mode, "keyed", o0, o1, x, xi, keyed, ys, xs, wy, wx, H, W, 2 * z[0, 0], 0)[0]
    assert np.array_equal(a, b)
    assert not np.array_equal(a, fused_step64(mode, "keyed", o0, o1, x, xi, keyed, ys, xs, wy, wx, H, W, z[0, 0], 5)[0])


@pytest.mark.parametrize("H,W,th,tw,overlap", PLANS[1:])
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_rows_cut_from_a_slice_give_the_slice_level_update(mode, H, W, th, tw, overlap):
    """tiles whose outputs are windows of ONE slice-level output blend back to it (a weighted mean of equal numbers, to float64's
    rounding), so every tile holds the window of the slice-level update"""
    ys, xs, wy, wx = _geometry(H, W, th, tw, overlap)
    g = np.random.default_rng(10 + mode)
    O0, O1, X, XI, Z = (g.standard_normal((H, W)) for _ in range(5))
    c = lambda a: cut(a, ys, xs, th, tw)
    for form, row, t in _forms(mode):
        rows, _, out = fused_step64(mode, form, c(O0), c(O1), c(X), c(XI), row, ys, xs, wy, wx, H, W, Z, t)
        want, _ = step64(mode, form, O0, O1, X, XI, row, Z, t)
        assert np.allclose(out, want, rtol=0, atol=1e-12) and np.allclose(rows, c(want), rtol=0, atol=1e-12)


@pytest.mark.parametrize("H,W,th,tw,overlap", PLANS[1:])
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_common_pixels_of_overlapping_tiles_are_identical(mode, H, W, th, tw, overlap):
    """the tiles' outputs disagree, their x_t and x_in are cut from one slice: after the step every covering tile holds the same
    number, which is the assembled slice's"""
    ys, xs, wy, wx = _geometry(H, W, th, tw, overlap)
    g = np.random.default_rng(20 + mode)
    X, XI, Z = (g.standard_normal((H, W)) for _ in range(3))
    o0, o1 = (g.standard_normal((len(ys), len(xs), th, tw)) for _ in range(2))
    for form, row, t in _forms(mode):
        rows, _, out = fused_step64(mode, form, o0, o1, cut(X, ys, xs, th, tw), cut(XI, ys, xs, th, tw), row, ys, xs, wy, wx, H, W, Z, t)
        assert np.array_equal(rows, cut(out, ys, xs, th, tw))
    # and they do differ from tile to tile when x_t is not the slice's
    rows, _, out = fused_step64(mode, "ddim", o0, o1, g.standard_normal(o0.shape), cut(XI, ys, xs, th, tw), _rows(0)[1], ys, xs, wy, wx, H, W)
    assert not np.array_equal(rows, cut(out, ys, xs, th, tw))


@pytest.mark.parametrize("H,W,th,tw,overlap", PLANS)
def test_noise_index_of_a_tile_pixel_is_the_slices(H, W, th, tw, overlap):
    """pixel (y, x) of the tile at (ya, xa) takes element p % 4 of the keyed stream's group p / 4, p = (ya + y) W + xa + x: the
    value oracle/keyed_noise.keyed_normal gives the slice there, whatever tile asks"""
    sys.path.insert(0, ROOT)
    from oracle.keyed_noise import keyed_normal
    ys, xs, _, _ = _geometry(H, W, th, tw, overlap)
    seed, t = 2 ** 40 + 7, 17
    field = keyed_normal(seed, t, H * W)
    groups = np.concatenate([field, np.zeros(-(H * W) % 4, dtype=np.float32)]).reshape(-1, 4)
    tiles = cut(field.reshape(H, W), ys, xs, th, tw)
    for iy, ya in enumerate(ys):
        for ix, xa in enumerate(xs):
            p = (ya + np.arange(th))[:, None] * W + xa + np.arange(tw)[None, :]
            assert np.array_equal(groups[p // 4, p % 4], tiles[iy, ix])
    if W % 4:                                                   # a lane's four pixels then lie in two groups
        p = ys[1] * W + xs[1]
        assert len({(p + e) // 4 for e in range(4)}) == 2 or len({(p + W + e) // 4 for e in range(4)}) == 2


def test_tile_owner():
    from founddiff_amd.tiling import tile_owner, tile_plan
    for H, W, th, tw, overlap in PLANS:
        ys, xs = tile_plan(H, th, overlap), tile_plan(W, tw, overlap)
        own = tile_owner(ys, xs, H, W, th, tw)
        assert own.shape == (H, W) and own.dtype == np.int64 and own.min() >= 0
        for y in range(H):
            for x in range(W):
                first = [iy * len(xs) + ix for iy, ya in enumerate(ys) for ix, xa in enumerate(xs)
                         if ya <= y < ya + th and xa <= x < xa + tw][0]
                assert own[y, x] == first, (y, x)
    assert tile_owner([0], [0], 8, 8, 8, 8).tolist() == np.zeros((8, 8), dtype=np.int64).tolist()
    assert (tile_owner([0], [0], 8, 10, 8, 8)[:, 8:] == -1).all()               # a pixel no tile covers
    own = tile_owner([0, 24, 32], [0, 24, 32], 64, 64, 32, 32)
    assert own[0, 0] == 0 and own[24, 24] == 0 and own[31, 32] == 1 and own[32, 31] == 3 and own[63, 63] == 8 and own[40, 40] == 4


def test_cabi_declares_the_entry_points():
    from founddiff_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "founddiff_hip.h")).read()
    for name, nargs in (("fd_tiles_step_ddim_f32", 21), ("fd_tiles_step_keyed_f32", 24)):
        assert name in hdr and len(L.SIGNATURES[name][1]) == nargs
    for build in (L.BF16, L.F16):
        lib = build.lib()
        assert hasattr(lib, "fd_tiles_step_ddim_f32") and hasattr(lib, "fd_tiles_step_keyed_f32")


def test_entries_reject_bad_arguments_without_launching():
    """null pointers, a mode's missing stream and fd_tiles.hip's shape limits fail in the entry itself, with a message"""
    from founddiff_amd import _lib as L
    one = 16                                                             # never dereferenced: every call fails its checks first
    ok = (1, 8, 8, 8, 8, 1, 1, 1)
    for build in (L.BF16, L.F16):
        lib = build.lib()
        ddim = lambda mode, o0, o1, x_t, x_in, par, geom, out: lib.fd_tiles_step_ddim_f32(
            mode, o0, o1, x_t, x_in, par, one, one, one, one, *geom, out, None, None)
        keyed = lambda mode, o0, o1, x_t, x_in, t_dev, seeds, geom, T: lib.fd_tiles_step_keyed_f32(
            mode, o0, o1, x_t, x_in, one, t_dev, seeds, one, one, one, one, *geom, one, None, T, None)
        for B, H, W, th, tw, my, mx in ((1, 8, 8, 9, 8, 1, 1), (1, 8, 8, 8, 9, 1, 1), (1, 8, 8, 8, 8, 0, 1), (1, 8, 8, 8, 8, 1, 0),
                                        (65536, 8, 8, 8, 8, 1, 1), (8192, 8, 8, 8, 8, 4, 2), (1, 32769, 8, 8, 8, 1, 1)):
            assert ddim(0, one, None, one, one, one, (B, H, W, th, tw, my, mx, 1), one) != 0
            assert b"fd_tiles_step_ddim_f32: unsupported shape" in lib.fd_last_error()
            assert keyed(0, one, None, one, one, one, one, (B, H, W, th, tw, my, mx, 1), 1000) != 0
            assert b"fd_tiles_step_keyed_f32: unsupported shape" in lib.fd_last_error()
        assert ddim(0, one, None, None, one, one, ok, one) != 0 and b"fd_tiles_step_ddim_f32: null pointer" in lib.fd_last_error()
        assert ddim(0, one, None, one, one, None, ok, one) != 0 and b"null pointer" in lib.fd_last_error()
        assert ddim(0, one, None, one, one, one, ok, None) != 0 and b"null pointer" in lib.fd_last_error()
        assert keyed(0, one, None, one, one, None, one, ok, 1000) != 0 and b"fd_tiles_step_keyed_f32: null pointer" in lib.fd_last_error()
        assert keyed(0, one, None, one, one, one, None, ok, 1000) != 0 and b"null pointer" in lib.fd_last_error()
        assert keyed(0, one, None, one, one, one, one, ok, 0) != 0 and b"bad table size" in lib.fd_last_error()
        for mode, o0, o1, x_in in ((0, None, one, one), (3, None, one, one), (1, one, None, one), (2, one, None, one), (2, None, one, one),
                                   (0, one, None, None), (1, None, one, None), (3, one, None, None)):
            assert ddim(mode, o0, o1, one, x_in, one, ok, one) != 0 and b"needs o0=" in lib.fd_last_error(), mode
            assert keyed(mode, o0, o1, one, x_in, one, one, ok, 1000) != 0 and b"needs o0=" in lib.fd_last_error(), mode
        for mode in (-1, 4):
            assert ddim(mode, one, one, one, one, one, ok, one) != 0 and b"bad mode" in lib.fd_last_error()


def test_fuse_argument_is_checked_before_any_work():
    """sample_tiled's host-side checks need no device: an unknown `fuse` raises, and fuse="step" keeps input_condition's refusal"""
    import inspect
    from founddiff_amd import parallel
    from founddiff_amd.DADiff import ResidualDiffusion, Trainer
    # `fuse` is keyword-only and taken in front of the method (DADiff._fuse_keyword), whose own parameter list stays the one
    # tests/test_tiling_cpu.py pins; its default is the mode the method runs without it
    assert "fuse" not in inspect.signature(ResidualDiffusion.sample_tiled).parameters
    assert 'fuse="final" (the default)' in ResidualDiffusion.sample_tiled.__doc__
    assert inspect.signature(Trainer.test).parameters["tile_fuse"].default == "final"
    assert inspect.signature(parallel.sample_volume).parameters["tile_fuse"].default == "final"

    class _Stub:
        input_condition = False
    with pytest.raises(RuntimeError, match="fuse must be 'final' or 'step'"):
        ResidualDiffusion.sample_tiled.__wrapped__(_Stub(), [None], 32, fuse="each")
    _Stub.input_condition = True
    stub = _Stub()
    with pytest.raises(RuntimeError, match="input_condition"):
        ResidualDiffusion.sample_tiled.__wrapped__(stub, [None], 32, fuse="step")
    assert stub._tile_fuse == "final"                          # the mode does not outlive the call, even one that raises
