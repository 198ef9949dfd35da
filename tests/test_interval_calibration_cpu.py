"""Calibrated intervals without a GPU: ensemble.risk_control on hand-built counts, the bin rule of the oracle, interval_grid, the grid
checks of metrics.interval_hist, a fixed-seed statistical check of the whole rule on the numpy oracle, the C ABI of
fd_interval_hist_f32 / fd_interval_scale_f32 and the argument checks of Trainer.calibrate_intervals and
Trainer.test(interval_scale=...)."""
import inspect
import math
import os
from fractions import Fraction

import numpy as np
import pytest

import interval_cases as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIST, SCALE = "fd_interval_hist_f32", "fd_interval_scale_f32"

# four slices of 10 pixels over the grid (0.5, 1, 2, 4); bins 0..4.  cum per slice at g = 0..3:
#   slice 0: 4 7 9 10   slice 1: 5 8 10 10   slice 2: 3 6 9 10   slice 3: 4 7 10 10   -> covered 16 28 38 40, missed 24 12 2 0
HAND = np.array([[4, 3, 2, 1, 0], [5, 3, 2, 0, 0], [3, 3, 3, 1, 0], [4, 3, 3, 0, 0]], np.int64)
HAND_GRID = (0.5, 1.0, 2.0, 4.0)


def test_risk_control_hand_case_crc():
    """R = 24/40, 12/40, 2/40, 0.  CRC at N = 4: (4 R + 1) / 5 = 0.68, 0.44, 0.24, 0.2"""
    from founddiff_amd.ensemble import IntervalCalibration, risk_control
    cal = risk_control(HAND, 10, HAND_GRID, 0.25)
    assert isinstance(cal, IntervalCalibration)
    assert (cal.g, cal.scale, cal.risk, cal.raw_risk, cal.grid_max) == (2, 2.0, 2 / 40, 12 / 40, 4.0)
    assert (cal.alpha, cal.bound, cal.delta, cal.n_slices, cal.n_pixels, cal.settings) == (0.25, "crc", None, 4, 10, None)
    assert risk_control(HAND, 10, HAND_GRID, 0.2).g == 3                 # 1/5 <= 0.2: equality is accepted, as the decimal reads
    assert risk_control(HAND, 10, HAND_GRID, 0.24).g == 2                # 6/25 <= 0.24
    assert risk_control(HAND, 10, HAND_GRID, 0.5).g == 1
    assert risk_control(HAND, 10, HAND_GRID, 0.7).g == 0
    assert risk_control(HAND.tolist(), 10, HAND_GRID, 0.25).g == 2       # lists of Python integers too
    assert risk_control(HAND, 10, (2.0, 4.0, 8.0, 16.0), 0.7).raw_risk is None


def test_risk_control_hand_case_hoeffding():
    """slack = sqrt(ln(1 / delta) / 8): delta = 0.5 -> 0.2944; R + slack = 0.894, 0.594, 0.344, 0.294"""
    from founddiff_amd.ensemble import risk_control
    slack = math.sqrt(math.log(2) / 8)
    assert 0.29 < slack < 0.30
    assert risk_control(HAND, 10, HAND_GRID, 0.35, bound="hoeffding", delta=0.5).g == 2
    assert risk_control(HAND, 10, HAND_GRID, 0.3, bound="hoeffding", delta=0.5).g == 3
    cal = risk_control(HAND, 10, HAND_GRID, 0.6, bound="hoeffding", delta=0.5)
    assert (cal.g, cal.scale, cal.delta, cal.bound) == (1, 1.0, 0.5, "hoeffding")


def test_risk_is_monotone_and_the_rational_formula():
    from founddiff_amd.ensemble import risk_control
    rng = np.random.default_rng(3)
    for N, n_pixels, G in ((1, 7, 1), (5, 100, 9), (12, 4096, 33)):
        counts = rng.multinomial(n_pixels, rng.dirichlet(np.ones(G + 1)), size=N)
        grid = np.linspace(0.25, 8, G)
        Rs = [ic.risk(counts, n_pixels, g) for g in range(G)]
        assert all(a >= b for a, b in zip(Rs, Rs[1:]))
        for alpha in (0.1, 0.3, 0.5, 0.9):
            want = ic.risk_control(counts, n_pixels, grid, alpha)
            if want is None:
                with pytest.raises(RuntimeError):
                    risk_control(counts, n_pixels, grid, alpha)
                continue
            cal = risk_control(counts, n_pixels, grid, alpha)
            assert (cal.g, cal.scale) == want[:2]
            assert cal.risk == want[2].numerator / want[2].denominator   # one rounding of the exact rational
            assert Fraction(cal.risk).limit_denominator(N * n_pixels) == want[2]
            raw = [g for g in range(G) if np.float32(grid[g]) <= 1]
            assert cal.raw_risk == (float(Rs[raw[-1]]) if raw else None)


def test_risk_control_failures():
    from founddiff_amd.ensemble import risk_control
    with pytest.raises(RuntimeError, match=r"too small for the bound: conformal risk control needs.*N >= 9 "):
        risk_control(HAND, 10, HAND_GRID, 0.1)
    with pytest.raises(RuntimeError, match=r"too small for the bound: the Hoeffding bound needs.*N >= 150 "):
        risk_control(HAND, 10, HAND_GRID, 0.1, bound="hoeffding", delta=0.05)          # ln 20 / 0.02 = 149.8
    short = HAND[:, :4].copy()
    short[:, 3] += HAND[:, 4]                                            # over the grid (0.5, 1, 2): R(2) = 2/40 -> 0.24 > 0.22 >= 1/5
    with pytest.raises(RuntimeError, match=r"the grid ends too early.*last value 2\.0.*R\(2\) = 0\.05 "):
        risk_control(short, 10, (0.5, 1.0, 2.0), 0.22)
    with pytest.raises(RuntimeError, match="needs 0 < delta < 1"):
        risk_control(HAND, 10, HAND_GRID, 0.5, bound="hoeffding")
    with pytest.raises(RuntimeError, match="delta belongs to bound='hoeffding'"):
        risk_control(HAND, 10, HAND_GRID, 0.5, delta=0.1)
    with pytest.raises(RuntimeError, match="bound must be"):
        risk_control(HAND, 10, HAND_GRID, 0.5, bound="bentkus")
    with pytest.raises(RuntimeError, match="sum to n_pixels"):
        risk_control(HAND, 11, HAND_GRID, 0.5)
    with pytest.raises(RuntimeError, match="integer array"):
        risk_control(HAND.astype(np.float64), 10, HAND_GRID, 0.5)
    with pytest.raises(RuntimeError, match="integer array"):
        risk_control(HAND, 10, HAND_GRID[:3], 0.5)


def test_bin_rule_of_the_oracle():
    grid = ic.GRIDS[33]
    m, l, u = (np.full(8, v, np.float32) for v in (0.5, 0.375, 0.75))
    y = np.array([0.5, 0.5 - 0.5 * 0.125, 0.5 + 0.5 * 0.25, 0.5 - 16 * 0.125, 0.5 + 16 * 0.25, np.nan, np.inf, 0.5 + 0.25 * 0.51],
                 np.float32)
    s, out = ic.score(m, l, u, y)
    assert s[:5].tolist() == [0.0, 0.5, 0.5, 16.0, 16.0] and s[6] == np.inf and out.tolist() == [False] * 5 + [True, False, False]
    assert ic.bins(s, out, grid).tolist() == [0, 1, 1, 32, 32, 33, 33, 2]       # s == grid[g] -> g; 0 -> 0; NaN, +inf -> G
    assert ic.hist(m[None], l[None], u[None], y[None], grid).sum() == 8
    for which in range(3):                                               # a NaN in any map takes the pixel out
        maps = [m.copy(), l.copy(), u.copy()]
        maps[which][0] = np.nan
        s, out = ic.score(*maps, y)
        assert out[0] and ic.bins(s, out, grid)[0] == 33
    # the floor: l = m = u
    s, out = ic.score(*(np.full(1, 0.25, np.float32),) * 3, np.array([0.25 + 2 / 3000], np.float32))
    assert 1.99 < s[0] < 2.01


def test_interval_grid():
    from founddiff_amd.ensemble import interval_grid
    g = interval_grid()
    assert g.dtype == np.float32 and g.shape == (1025,) and g[0] == 0 and g[-1] == 16 and g[64] == 1.0
    assert np.array_equal(g, np.linspace(0, 16, 1025).astype(np.float32)) and (np.diff(g) > 0).all()
    g = interval_grid(4.0, 5)
    assert g.dtype == np.float32 and g.tolist() == [0, 1, 2, 3, 4]


def test_interval_hist_rejects_bad_grids_before_the_library(monkeypatch):
    from founddiff_amd import _lib as L
    from founddiff_amd import metrics

    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(L, "lib", boom)
    monkeypatch.setattr(L, "call", boom)
    for grid, words in (([1.0, 0.5], "strictly increasing"), ([1.0, 1.0], "strictly increasing"), ([-0.5, 1.0], "start at a value >= 0"),
                        ([0.5, float("nan")], "finite"), ([0.5, float("inf")], "finite"), ([], "1 to 4096 values"),
                        (np.arange(4097), "1 to 4096 values")):
        with pytest.raises(RuntimeError, match="interval_hist: the grid must.*" + words):
            metrics.interval_hist(None, None, None, None, grid)
    with pytest.raises(RuntimeError, match="floor must be positive"):
        metrics.interval_hist(None, None, None, None, [1.0], floor=0.0)
    with pytest.raises(RuntimeError, match="scale must be non-negative"):
        metrics.interval_scale(None, None, None, -1.0)
    assert metrics.INTERVAL_FLOOR == 1 / 3000


def test_toy_model_raw_interval_undercovers_and_the_calibrated_one_does_not():
    """K = 8 exchangeable clamped normal draws plus one truth per pixel, a third of the pixels air, 64 calibration and 64 test slices
    of 64 x 64, alpha = 0.1, CRC, the default grid: the raw [q0.05, q0.95] misses more than alpha of the test pixels, the calibrated
    one at most alpha."""
    from founddiff_amd.ensemble import interval_grid, risk_control
    rng = np.random.default_rng(0)
    grid, alpha = interval_grid(), 0.1
    cal_maps, test_maps = ic.toy_slices(rng, 64), ic.toy_slices(rng, 64)
    cal = risk_control(ic.hist(*cal_maps, grid), 64 * 64, grid, alpha)
    s, out = ic.score(*test_maps)
    raw_miss = float(np.mean(out | (s > np.float32(1.0))))
    cal_miss = float(np.mean(out | (s > np.float32(cal.scale))))
    print(f"toy model: raw miss {raw_miss:.4f}, scale {cal.scale:.4f}, calibrated miss {cal_miss:.4f}, calibration risk {cal.risk:.4f}")
    assert cal.raw_risk > alpha and raw_miss > alpha
    assert cal_miss <= alpha
    assert cal.scale > 1 and cal.risk <= alpha


# ---- the C ABI
def test_cabi_declares_the_entry_points():
    from founddiff_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "founddiff_hip.h")).read()
    for name, nargs in ((HIST, 16), ("fd_interval_hist_nblk", 1), (SCALE, 15), ("fd_interval_scale_nblk", 1)):
        assert "int " + name + "(" in hdr, name
        assert len(L.SIGNATURES[name][1]) == nargs, name
    for build in (L.BF16, L.F16):
        lib = build.lib()
        assert [lib.fd_interval_hist_nblk(n) for n in (4, 1025, 72 * 72, 512 * 512)] == [1, 2, 6, 64]
        assert [lib.fd_interval_scale_nblk(n) for n in (4, 1025, 512 * 512)] == [1, 2, 256]
        for f in (lib.fd_interval_hist_nblk, lib.fd_interval_scale_nblk):
            assert f(0) == 0 and f(-4) == 0 and f(1 << 34) == 0


def test_entries_reject_bad_arguments_without_launching():
    from founddiff_amd import _lib as L
    one = 16                                                             # never dereferenced: every call fails its checks first
    for build in (L.BF16, L.F16):
        lib = build.lib()

        def hist(ptrs=(one,) * 7, strides=(64, 64, 64, 64), G=3, floor=1 / 3000, B=1, n=64):
            ce, lo, hi, tg, grid, ws, out = ptrs
            return lib.fd_interval_hist_f32(ce, strides[0], lo, strides[1], hi, strides[2], tg, strides[3], grid, G, floor, ws, out,
                                            B, n, None)

        def scale(ptrs=(one,) * 7, strides=(64, 64, 64), s=1.0, floor=1 / 3000, B=1, n=64):
            ce, lo, hi, lo_out, hi_out, ws, width = ptrs
            return lib.fd_interval_scale_f32(ce, strides[0], lo, strides[1], hi, strides[2], s, floor, lo_out, hi_out, ws, width, B,
                                             n, None)
        for fn, name in ((hist, HIST), (scale, SCALE)):
            for i in range(7):
                p = [one] * 7
                p[i] = None
                assert fn(ptrs=p) != 0 and (name + ": null pointer").encode() in lib.fd_last_error(), (name, i)
            for kw in (dict(B=0), dict(B=65536), dict(n=0), dict(n=-1), dict(n=1 << 34), dict(strides=(-4, 64, 64, 64)[:4 if fn is hist else 3])):
                assert fn(**kw) != 0 and (name + ": unsupported shape").encode() in lib.fd_last_error(), (name, kw)
            for kw in (dict(floor=0.0), dict(floor=-1.0), dict(floor=float("inf")), dict(floor=float("nan"))):
                assert fn(**kw) != 0 and (name + ": floor must be positive").encode() in lib.fd_last_error(), (name, kw)
        for kw in (dict(G=0), dict(G=4097), dict(strides=(64, 64, 64, -1))):
            assert hist(**kw) != 0 and b"fd_interval_hist_f32: unsupported shape" in lib.fd_last_error(), kw
        for s in (-0.5, float("inf"), float("nan")):
            assert scale(s=s) != 0 and b"fd_interval_scale_f32: floor must be positive, scale non-negative" in lib.fd_last_error(), s


@pytest.mark.parametrize("half", ["bf16", "fp16"])
def test_kernels_use_no_scratch_and_no_agprs(half):
    from founddiff_amd import build
    tab = build.resources(half).get("fd_interval.hip")
    assert tab, "no resource report for fd_interval.hip"
    for vec in ("Lb1", "Lb0"):                                           # the 16-byte and the scalar form
        for kernel in ("interval_hist_kernel", "interval_scale_kernel"):
            assert len([k for k in tab if f"{kernel}I{vec}E" in k]) == 1, (kernel, vec)
    assert len([k for k in tab if "interval_hist_finish_kernel" in k]) == 1 and len([k for k in tab if "interval_width_kernel" in k]) == 1
    assert len(tab) == 6
    for name, r in tab.items():
        assert r["scratch"] == 0 and r["agpr"] == 0, (name, r)
        if "interval_hist_kernel" in name:
            assert r["lds"] == 2 * 16384, (name, r)                      # the grid and the counters, no more


# ---- the host side
def test_public_interface():
    from founddiff_amd import ensemble, metrics
    from founddiff_amd.DADiff import Trainer
    assert ensemble.IntervalCalibration._fields == ("scale", "g", "alpha", "bound", "delta", "n_slices", "n_pixels", "risk", "raw_risk",
                                                    "grid_max", "settings")
    assert list(inspect.signature(metrics.interval_hist).parameters) == ["center", "lo", "hi", "target", "grid", "floor"]
    assert list(inspect.signature(metrics.interval_scale).parameters) == ["center", "lo", "hi", "scale", "floor"]
    assert list(inspect.signature(ensemble.risk_control).parameters) == ["hist", "n_pixels", "grid", "alpha", "bound", "delta"]
    kw = inspect.Parameter.KEYWORD_ONLY
    p = inspect.signature(Trainer.test).parameters
    assert p["interval_scale"].kind is kw and p["interval_scale"].default is None
    assert p["orientations"].kind is kw and p["tiled_ensemble"].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
    p = inspect.signature(Trainer.calibrate_intervals).parameters
    assert list(p) == ["self", "dataset", "n_samples", "quantiles", "estimate", "alpha", "bound", "delta", "grid", "floor", "ensemble_seed",
                       "batch_size", "items", "tile", "overlap", "tile_condition", "tile_fuse", "tiled_ensemble", "orientations"]
    assert p["dataset"].default is None and all(v.kind is kw for k, v in p.items() if k not in ("self", "dataset"))
    assert p["n_samples"].default is inspect.Parameter.empty and p["quantiles"].default is inspect.Parameter.empty
    assert (p["alpha"].default, p["bound"].default, p["floor"].default, p["batch_size"].default) == (0.1, "crc", 1 / 3000, 1)
    assert list(inspect.signature(Trainer.load_interval_calibration).parameters) == ["self", "path"]


def test_arguments_are_checked_before_any_work():
    """the host-side checks need no device and no trainer: a bare object stands in for self"""
    from founddiff_amd.DADiff import Trainer
    test = Trainer.test.__wrapped__
    cal = Trainer.calibrate_intervals.__wrapped__
    with pytest.raises(RuntimeError, match="Trainer.test: interval_scale needs quantiles with at least two levels"):
        test(object(), n_samples=3, interval_scale=2.0)
    with pytest.raises(RuntimeError, match="Trainer.test: interval_scale needs quantiles with at least two levels"):
        test(object(), n_samples=3, quantiles=(0.5,), interval_scale="calibrated")
    with pytest.raises(RuntimeError, match="need an ensemble, n_samples > 1"):
        test(object(), quantiles=(0.05, 0.95), interval_scale=2.0)
    with pytest.raises(RuntimeError, match="needs a calibration: call calibrate_intervals or load_interval_calibration"):
        test(object(), n_samples=3, quantiles=(0.05, 0.95), interval_scale="calibrated")
    for bad in ("auto", -1.0, float("nan"), float("inf"), True, [2.0]):
        with pytest.raises(RuntimeError, match="interval_scale must be None, a number"):
            test(object(), n_samples=3, quantiles=(0.05, 0.95), interval_scale=bad)
    # calibrate_intervals refuses what test() refuses, in the same words
    good = dict(n_samples=3, quantiles=(0.05, 0.95))
    for kw, words in ((dict(n_samples=1), "need an ensemble, n_samples > 1"), (dict(n_samples=0), "n_samples must be at least 1"),
                      (dict(estimate="mode"), "estimate must be 'mean' or 'median'"), (dict(quantiles=(0.05, 0.0501)), "collide"),
                      (dict(quantiles=(-0.1, 0.5)), "quantile_table: levels must be finite"),
                      (dict(tile=8), "ensembles of tiled samples.*tiled_ensemble=True"),
                      (dict(tile=8, orientations="flips"), "orientation ensembles of tiled samples are not built")):
        with pytest.raises(RuntimeError, match=words):
            cal(object(), **dict(good, **kw))
        with pytest.raises(RuntimeError, match=words):
            test(object(), **dict(good, **kw))
    for kw, words in ((dict(quantiles=(0.5,)), "at least two levels"), (dict(quantiles=None), "at least two levels"),
                      (dict(grid=[1.0, 0.5]), "strictly increasing"), (dict(floor=0.0), "floor must be positive"),
                      (dict(alpha=0.0), "need 0 < alpha < 1"), (dict(bound="hoeffding"), "'hoeffding' with 0 < delta < 1"),
                      (dict(delta=0.1), "'hoeffding' with 0 < delta < 1"), (dict(batch_size=0), "batch_size must be an integer >= 1"),
                      (dict(items=0), "items None or an integer >= 1")):
        with pytest.raises(RuntimeError, match="Trainer.calibrate_intervals: .*" + words if "increasing" not in words else words):
            cal(object(), **dict(good, **kw))
    with pytest.raises(RuntimeError, match="Trainer.calibrate_intervals: no dataset"):
        cal(object(), **good)
    with pytest.raises(TypeError):                                       # keyword-only
        cal(object(), None, 3, (0.05, 0.95))
