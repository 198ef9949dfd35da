"""Orientation ensembles without a GPU: ensemble.orientation_inverse and orientation_codes against
diffusion_train.augment_source_index, the C ABI of the three entries of csrc/fd_ensemble_orient.hip (declared, bound, exported by
both builds, bad arguments rejected before any launch), their kernels' resources, and the host-side checks of the new keyword."""
import inspect
import itertools

import numpy as np
import pytest

ORIENT, STATS, TAKE = "fd_rows_orient_f32", "fd_ensemble_orient_stats_f32", "fd_rows_take_f32"


def _maps(code, n=5):
    from founddiff_amd.diffusion_train import augment_source_index
    return augment_source_index(code, n, n)


# ---- the host definitions
def test_inverse_undoes_every_code():
    from founddiff_amd.ensemble import orientation_inverse
    y, x = np.meshgrid(np.arange(5), np.arange(5), indexing="ij")
    for code in range(16):
        inv = orientation_inverse(code)
        assert 0 <= inv <= 7
        i1, j1 = _maps(code)                   # out1[y, x] = m[i1, j1]
        i2, j2 = _maps(inv)                    # out2[y, x] = out1[i2, j2] = m[i1[i2, j2], j1[i2, j2]]
        assert np.array_equal(i1[i2, j2], y) and np.array_equal(j1[i2, j2], x), code
        # and on an image: the numpy transform of the documentation
        m = np.arange(25.0).reshape(5, 5)
        t = m[i1, j1]
        f = m[::-1] if code & 1 else m
        f = f[:, ::-1] if code & 2 else f
        assert np.array_equal(t, np.rot90(f, (code >> 2) & 3)), code
        assert np.array_equal(t[i2, j2], m), code
    for bad in (-1, 16, 2.5, "d4"):
        with pytest.raises(RuntimeError):
            orientation_inverse(bad)


def test_codes_0_to_7_are_the_eight_elements():
    from founddiff_amd.ensemble import ORIENTATIONS_D4, ORIENTATIONS_FLIPS, orientation_inverse
    assert ORIENTATIONS_D4 == tuple(range(8)) and ORIENTATIONS_FLIPS == (0, 1, 2, 3)
    flat = [np.stack(_maps(c)).tobytes() for c in range(16)]
    for a, b in itertools.combinations(range(8), 2):
        assert flat[a] != flat[b], (a, b)
    for c in range(8, 16):                     # the second eight reach the same elements: inverse of inverse names the twin
        twin = orientation_inverse(orientation_inverse(c))
        assert 0 <= twin <= 7 and flat[twin] == flat[c], c
    for c in range(8):
        assert orientation_inverse(orientation_inverse(c)) == c
    for c in ORIENTATIONS_FLIPS:               # what keeps an H != W shape, and is its own inverse
        from founddiff_amd.diffusion_train import augment_source_index
        assert augment_source_index(c, 3, 7)[0].shape == (3, 7) and orientation_inverse(c) == c


def test_orientation_codes():
    from founddiff_amd.ensemble import orientation_codes
    c = orientation_codes("d4", 8, True)
    assert c.dtype == np.int32 and c.tolist() == list(range(8))
    assert orientation_codes("d4", 16, True).tolist() == list(range(8)) * 2             # every orientation under two seeds
    assert orientation_codes("d4", 3, True).tolist() == [0, 1, 2]
    assert orientation_codes("flips", 6, False).tolist() == [0, 1, 2, 3, 0, 1]
    assert orientation_codes("flips", 2, True).tolist() == [0, 1]
    assert orientation_codes((5, 12, 3), 7, True).tolist() == [5, 12, 3, 5, 12, 3, 5]
    assert orientation_codes([2], 3, False).tolist() == [2, 2, 2]
    assert orientation_codes(np.array([8, 11]), 2, False).tolist() == [8, 11]           # k = 2: no transpose
    with pytest.raises(RuntimeError, match="flips"):
        orientation_codes("d4", 8, False)
    for bad in ((0, 4), (13,), [7, 0]):
        with pytest.raises(RuntimeError, match="square"):
            orientation_codes(bad, 2, False)
    for bad in ("d8", (), [], (16,), (-1,), (1.5,), (True,), ("1",), 3, None):
        with pytest.raises(RuntimeError):
            orientation_codes(bad, 2, True)
    with pytest.raises(RuntimeError):
        orientation_codes("d4", 0, True)


# ---- the C ABI
def test_entries_are_declared_bound_and_exported():
    import os
    import re
    from founddiff_amd import _lib as L
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "founddiff_hip.h")).read()
    for name in (ORIENT, STATS, TAKE):
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in L.SIGNATURES
        for build in (L.BF16, L.F16):
            assert hasattr(build.lib(), name)
    assert len(L.SIGNATURES[ORIENT][1]) == 8 and len(L.SIGNATURES[STATS][1]) == 12 and len(L.SIGNATURES[TAKE][1]) == 6


def test_entries_reject_bad_arguments_without_launching():
    from founddiff_amd import _lib as L
    one = 16                                                             # never dereferenced: every call fails its checks first
    for build in (L.BF16, L.F16):
        lib = build.lib()
        for i in range(3):
            p = [one] * 3
            p[i] = None
            assert lib.fd_rows_orient_f32(*p, 1, 1, 8, 8, None) != 0 and b"fd_rows_orient_f32: null pointer" in lib.fd_last_error()
            assert lib.fd_rows_take_f32(*p, 1, 8, None) != 0 and b"fd_rows_take_f32: null pointer" in lib.fd_last_error()
        for B, K, H, W in ((0, 1, 8, 8), (65536, 1, 8, 8), (1, 0, 8, 8), (1, 65536, 8, 8), (1, 1, 0, 8), (1, 1, 8, 32769), (1, 1, -4, 8)):
            assert lib.fd_rows_orient_f32(one, one, one, B, K, H, W, None) != 0
            assert b"fd_rows_orient_f32: unsupported shape" in lib.fd_last_error(), (B, K, H, W)
            assert lib.fd_ensemble_orient_stats_f32(one, one, one, one, one, one, None, B, K, H, W, None) != 0
            assert b"fd_ensemble_orient_stats_f32: unsupported shape" in lib.fd_last_error(), (B, K, H, W)
        for i in range(6):                                               # samples_out alone may be NULL
            p = [one] * 6
            p[i] = None
            assert lib.fd_ensemble_orient_stats_f32(*p, None, 1, 2, 8, 8, None) != 0
            assert b"fd_ensemble_orient_stats_f32: null pointer" in lib.fd_last_error(), i
        for R, n in ((0, 8), (-1, 8), (1, 0), (1, 1 << 40)):
            assert lib.fd_rows_take_f32(one, one, one, R, n, None) != 0 and b"fd_rows_take_f32: unsupported shape" in lib.fd_last_error()


@pytest.mark.parametrize("half", ["bf16", "fp16"])
def test_kernels_use_no_scratch_and_no_agprs(half):
    from founddiff_amd import build
    tab = build.resources(half).get("fd_ensemble_orient.hip")
    assert tab, "no resource report for fd_ensemble_orient.hip"
    for kernel in ("rows_orient_kernel", "orient_stats_kernel", "orient_std_kernel", "rows_take_kernel"):
        for vec in ("Lb1", "Lb0"):                                       # the 16-byte and the scalar form
            assert len([k for k in tab if f"{kernel}I{vec}E" in k]) == 1, (kernel, vec)
    assert len([k for k in tab if "orient_finish_kernel" in k]) == 1
    assert len(tab) == 10                                                # and the partial sum this file instantiates
    for name, r in tab.items():
        assert r["scratch"] == 0 and r["agpr"] == 0, (name, r)
    for name, r in tab.items():                                          # the padded tile, only where 16-byte reads can transpose
        if "rows_orient_kernelILb1E" in name or "orient_stats_kernelILb1E" in name:
            assert r["lds"] == 64 * 65 * 4, (name, r)


# ---- the public interface
def test_public_interface():
    from founddiff_amd import ensemble, parallel
    from founddiff_amd.DADiff import ResidualDiffusion, Trainer
    kw = inspect.Parameter.KEYWORD_ONLY
    for fn in (ResidualDiffusion.sample_ensemble, Trainer.test, parallel.sample_volume):
        p = inspect.signature(fn).parameters
        assert p["orientations"].kind is kw and p["orientations"].default is None, fn
    assert list(inspect.signature(ensemble.orientation_codes).parameters) == ["orientations", "K", "square"]
    assert list(inspect.signature(ensemble.orientation_inverse).parameters) == ["code"]


def test_arguments_are_checked_before_any_work():
    """the host-side checks of the new keyword need no device"""
    import torch
    from founddiff_amd import parallel
    from founddiff_amd.DADiff import ResidualDiffusion, Trainer

    class _Stub:
        input_condition = False
    run = ResidualDiffusion.sample_ensemble.__wrapped__
    sq, wide = torch.zeros(1, 1, 8, 8), torch.zeros(1, 1, 8, 24)
    with pytest.raises(RuntimeError, match="orientation ensembles of tiled samples are not built"):
        run(_Stub(), [sq], 2, tile=8, orientations="d4")
    with pytest.raises(RuntimeError, match="orientation ensembles of tiled samples are not built"):
        run(_Stub(), [sq], 2, tile=8, orientations="flips", quantiles=(0.5,))
    with pytest.raises(RuntimeError, match="flips"):
        run(_Stub(), [wide], 8, orientations="d4")
    with pytest.raises(RuntimeError, match="square"):
        run(_Stub(), [wide], 2, orientations=(0, 5))
    with pytest.raises(RuntimeError, match="0..15"):
        run(_Stub(), [sq], 2, orientations=(0, 16))
    with pytest.raises(RuntimeError, match=r"x_input must be \[ldct"):
        run(_Stub(), [None], 2, orientations="d4")
    with pytest.raises(TypeError):                                       # keyword-only
        run(_Stub(), [sq], 2, None, False, "d4")
    _Stub.input_condition = True
    with pytest.raises(RuntimeError, match="input_condition"):
        run(_Stub(), [sq], 2, orientations="d4")
    with pytest.raises(RuntimeError, match="orientation ensembles of tiled samples are not built"):
        Trainer.test.__wrapped__(None, tile=32, orientations="d4")
    with pytest.raises(RuntimeError, match="orientation ensembles of tiled samples are not built"):
        parallel.sample_volume(None, sq, tile=8, orientations="flips")
