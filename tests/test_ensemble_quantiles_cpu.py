"""Ensemble quantiles without a GPU: ensemble.quantile_table against hand values and numpy.quantile, the C ABI of fd_ensemble_order_f32
and fd_ensemble_coverage_f32 (declared, exported by both builds, arguments checked before any launch), the resource report of their
kernels, and the new keywords of sample_ensemble, Trainer.test and sample_volume."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDER, COVERAGE, NBLK = "fd_ensemble_order_f32", "fd_ensemble_coverage_f32", "fd_ensemble_coverage_nblk"


def _table(levels, K):
    from founddiff_amd.ensemble import quantile_table
    lo, hi, frac = quantile_table(levels, K)
    assert lo.dtype == np.int32 and hi.dtype == np.int32 and frac.dtype == np.float32
    return list(zip(lo.tolist(), hi.tolist(), frac.tolist()))


# ---- quantile_table
def test_table_hand_values():
    assert _table([0, 0.05, 0.5, 1], 1) == [(0, 0, 0.0)] * 4
    assert _table([0.5], 5) == [(2, 3, 0.0)]
    assert _table([0.5], 4) == [(1, 2, 0.5)]
    for K in (1, 2, 7, 33):
        assert _table([1], K) == [(K - 1, K - 1, 0.0)]
        assert _table([0], K) == [(0, min(1, K - 1), 0.0)]
    assert _table([0.1], 11) == [(1, 2, 0.0)]                            # 0.1 * 10 snaps to 1
    assert _table([0.3], 11) == [(3, 4, 0.0)]                            # 0.3 * 10 = 3.0000000000000004 in float64
    assert _table([0.7], 11) == [(7, 8, 0.0)]                            # 0.7 * 10 = 7.000000000000001
    assert _table([0.25], 4) == [(0, 1, 0.75)]
    # the caller's order, duplicates allowed
    assert _table([1, 0.5, 0.5, 0], 3) == [(2, 2, 0.0), (1, 2, 0.0), (1, 2, 0.0), (0, 1, 0.0)]


def test_table_is_numpys_linear_rule():
    """Against numpy.quantile(method="linear") on random float64 data, K = 1 .. 40, a dozen levels, to 1e-12.  The table's frac is
    a float32, so v_lo + frac (v_hi - v_lo) with the RETURNED frac can be 2^-24 |v_hi - v_lo| off, far above 1e-12, unless frac is
    exact in float32.  So: the seven dyadic levels (frac a multiple of 1/8: exact) are compared with the returned frac; every
    level is compared with lo, hi and the float64 h - lo, and its returned frac must be float32(h - lo) exactly."""
    from founddiff_amd.ensemble import quantile_table
    rng = np.random.default_rng(0)
    dyadic = [0, 0.125, 0.25, 0.5, 0.75, 0.875, 1]
    others = [0.01, 0.05, 0.1, 1 / 3, 0.9, 0.95]
    assert len(dyadic + others) >= 12
    for K in range(1, 41):
        v = np.sort(rng.standard_normal(K))
        for part in (dyadic, others):
            lo, hi, frac = quantile_table(part, K)
            assert (0 <= lo).all() and (lo <= hi).all() and (hi <= K - 1).all() and (0 <= frac).all() and (frac <= 1).all()
            ref = np.quantile(v, part, method="linear")
            h = np.asarray(part, dtype=np.float64) * (K - 1)
            h = np.where(np.abs(h - np.rint(h)) <= 1e-9, np.rint(h), h)
            assert np.array_equal(frac, (h - lo).astype(np.float32)), (K, part)
            assert np.abs(v[lo] + (h - lo) * (v[hi] - v[lo]) - ref).max() <= 1e-12, (K, part)
            if part is dyadic:
                assert np.abs(v[lo] + frac.astype(np.float64) * (v[hi] - v[lo]) - ref).max() <= 1e-12, K


def test_table_errors():
    from founddiff_amd.ensemble import quantile_table
    for K in (0, -2):
        with pytest.raises(RuntimeError, match="quantile_table: K must be at least 1"):
            quantile_table([0.5], K)
    for levels in ([], [0.1] * 9):
        with pytest.raises(RuntimeError, match="quantile_table: 1 to 8 levels"):
            quantile_table(levels, 5)
    for bad in (-0.01, 1.01, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match="quantile_table: levels must be finite and in"):
            quantile_table([0.5, bad], 5)


def test_suffixes():
    from founddiff_amd.ensemble import quantile_suffix
    assert quantile_suffix([0.05, 0.5, 0.95, 0, 1, 0.0254]) == ["_q0050", "_q0500", "_q0950", "_q0000", "_q1000", "_q0025"]
    with pytest.raises(RuntimeError, match="collide"):
        quantile_suffix([0.05, 0.0501])


# ---- the C ABI
def test_cabi_declares_the_entry_points():
    from founddiff_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "founddiff_hip.h")).read()
    for name, nargs in ((ORDER, 10), (NBLK, 1), (COVERAGE, 11)):
        assert "int " + name + "(" in hdr, name
        assert len(L.SIGNATURES[name][1]) == nargs, name
        for build in (L.BF16, L.F16):
            assert hasattr(build.lib(), name), name
    for build in (L.BF16, L.F16):
        lib = build.lib()
        assert lib.fd_ensemble_coverage_nblk(4) == 1 and lib.fd_ensemble_coverage_nblk(1025) == 2
        assert lib.fd_ensemble_coverage_nblk(512 * 512) == 256
        assert lib.fd_ensemble_coverage_nblk(0) == 0 and lib.fd_ensemble_coverage_nblk(-4) == 0 and lib.fd_ensemble_coverage_nblk(1 << 40) == 0


def _arr(ctype, vals):
    return (ctype * len(vals))(*vals)


def test_order_rejects_bad_arguments_without_launching():
    from founddiff_amd import _lib as L
    one = 16                                                             # never dereferenced: every call fails its checks first
    for build in (L.BF16, L.F16):
        lib = build.lib()

        def call(samples=one, out=one, lo=(0, 2), hi=(1, 4), frac=(0.5, 0.0), B=1, K=5, Q=2, n=64):
            tab = [None if t is None else _arr(c, t) for c, t in ((L.i32, lo), (L.i32, hi), (L.f32, frac))]
            return lib.fd_ensemble_order_f32(samples, out, *tab, B, K, Q, n, None)
        for kw in (dict(samples=None), dict(out=None), dict(lo=None), dict(hi=None), dict(frac=None)):
            assert call(**kw) != 0 and b"fd_ensemble_order_f32: null pointer" in lib.fd_last_error(), kw
        for kw in (dict(K=0, lo=(0, 0), hi=(0, 0)), dict(K=-1), dict(K=65536), dict(Q=0), dict(Q=9, lo=(0,) * 9, hi=(0,) * 9, frac=(0.0,) * 9),
                   dict(B=0), dict(B=65536), dict(n=0), dict(n=-8), dict(n=1 << 40)):
            assert call(**kw) != 0 and b"fd_ensemble_order_f32: unsupported shape" in lib.fd_last_error(), kw
        for kw in (dict(lo=(0, 3), hi=(1, 2)), dict(hi=(1, 5)), dict(lo=(-1, 2)), dict(frac=(0.5, -0.001)), dict(frac=(1.001, 0.0)),
                   dict(frac=(float("nan"), 0.0))):
            assert call(**kw) != 0 and b"fd_ensemble_order_f32: bad table row" in lib.fd_last_error(), kw


def test_coverage_rejects_bad_arguments_without_launching():
    from founddiff_amd import _lib as L
    one = 16
    for build in (L.BF16, L.F16):
        lib = build.lib()

        def call(ptrs=(one,) * 5, strides=(64, 64, 64), B=1, n=64):
            lo, hi, tg, ws, count = ptrs
            return lib.fd_ensemble_coverage_f32(lo, strides[0], hi, strides[1], tg, strides[2], ws, count, B, n, None)
        for i in range(5):
            p = [one] * 5
            p[i] = None
            assert call(ptrs=p) != 0 and b"fd_ensemble_coverage_f32: null pointer" in lib.fd_last_error(), i
        for kw in (dict(B=0), dict(B=-1), dict(B=65536), dict(n=0), dict(n=-1), dict(n=1 << 40), dict(strides=(-64, 64, 64)),
                   dict(strides=(64, 64, -1))):
            assert call(**kw) != 0 and b"fd_ensemble_coverage_f32: unsupported shape" in lib.fd_last_error(), kw


@pytest.mark.parametrize("half", ["bf16", "fp16"])
def test_kernels_use_no_scratch_and_no_agprs(half):
    from founddiff_amd import build
    tab = build.resources(half).get("fd_ensemble_order.hip")
    assert tab, "no resource report for fd_ensemble_order.hip"
    for vec in ("Lb1", "Lb0"):                                           # the 16-byte and the scalar form
        for P in (4, 8, 16, 32):                                         # the networks, per padded size
            assert len([k for k in tab if f"order_net_kernelI{vec}ELi{P}E" in k]) == 1, (vec, P)
        assert len([k for k in tab if f"order_rank_kernelI{vec}E" in k]) == 1, vec
        assert len([k for k in tab if f"coverage_kernelI{vec}E" in k]) == 1, vec
    assert len([k for k in tab if "coverage_finish_kernel" in k]) == 1
    assert len(tab) == 13
    for name, r in tab.items():
        assert r["scratch"] == 0 and r["agpr"] == 0, (name, r)


# ---- the host side
def test_public_interface():
    from founddiff_amd import metrics, parallel
    from founddiff_amd.DADiff import EnsembleQuantiles, EnsembleResult, ResidualDiffusion, Trainer
    assert EnsembleResult._fields == ("mean", "std", "spread", "samples")
    assert EnsembleQuantiles._fields == ("mean", "std", "spread", "samples", "quantiles", "levels")
    kw = inspect.Parameter.KEYWORD_ONLY
    p = inspect.signature(ResidualDiffusion.sample_ensemble).parameters
    assert p["quantiles"].kind is kw and p["quantiles"].default is None
    p = inspect.signature(Trainer.test).parameters
    assert p["quantiles"].kind is kw and p["quantiles"].default is None
    assert p["estimate"].kind is kw and p["estimate"].default == "mean"
    assert p["tiled_ensemble"].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD              # what was positional stays so
    p = inspect.signature(parallel.sample_volume).parameters
    assert p["quantiles"].kind is kw and p["quantiles"].default is None
    assert list(inspect.signature(metrics.ensemble_quantiles).parameters) == ["samples", "levels"]
    assert list(inspect.signature(metrics.interval_coverage).parameters) == ["lo", "hi", "target"]


def test_arguments_are_checked_before_any_work():
    """the host-side checks of the new keywords need no device"""
    import torch
    from founddiff_amd import parallel
    from founddiff_amd.DADiff import ResidualDiffusion, Trainer

    class _Stub:
        input_condition = False
    run = ResidualDiffusion.sample_ensemble.__wrapped__
    with pytest.raises(RuntimeError, match="quantile_table: levels must be finite"):
        run(_Stub(), [None], 3, quantiles=(0.5, 1.5))
    with pytest.raises(RuntimeError, match="quantile_table: 1 to 8 levels"):
        run(_Stub(), [None], 3, quantiles=())
    with pytest.raises(TypeError):                                       # keyword-only
        run(_Stub(), [None], 3, None, False, None, 0, "tile", "final", (0.5,))
    test = Trainer.test.__wrapped__
    for kw in (dict(quantiles=(0.05, 0.95)), dict(estimate="median"), dict(n_samples=1, estimate="median")):
        with pytest.raises(RuntimeError, match="need an ensemble, n_samples > 1"):
            test(object(), **kw)
    with pytest.raises(RuntimeError, match="estimate must be 'mean' or 'median'"):
        test(object(), n_samples=3, estimate="mode")
    with pytest.raises(RuntimeError, match="collide"):
        test(object(), n_samples=3, quantiles=(0.05, 0.0501))
    with pytest.raises(RuntimeError, match="quantile_table: levels must be finite"):
        test(object(), n_samples=3, quantiles=(-0.1,))
    with pytest.raises(RuntimeError, match="ensembles of tiled samples.*tiled_ensemble=True"):       # the raise of before stays
        test(object(), n_samples=3, tile=8, quantiles=(0.5,))

    class _Dif:
        def parameters(self):
            return iter([torch.zeros(1)])
    for n_samples in (1, 0):
        with pytest.raises(RuntimeError, match="sample_volume: quantiles need an ensemble"):
            parallel.sample_volume(_Dif(), torch.zeros(2, 1, 8, 8), n_samples=n_samples, quantiles=(0.5,))
