"""Tiled ensembles without a GPU: tiling.tiled_ensemble_seeds against its definition, the C ABI of fd_tiles_ensemble_f32 (declared,
exported by both builds, arguments checked before any launch), the resource report of its kernels, and the host-side arguments of
sample_ensemble(tile=...) and of its callers."""
import inspect
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "fd_tiles_ensemble_f32"


def test_seeds_are_replica_first_then_tile():
    from founddiff_amd.ensemble import ensemble_seeds
    from founddiff_amd.tiling import tile_seeds, tiled_ensemble_seeds
    s = [3, 2 ** 40 + 5, 2 ** 62 - 1]
    t = tiled_ensemble_seeds(s, 4, 9)
    assert t.shape == (3, 4, 9) and t.dtype == np.int64
    assert np.array_equal(t, tile_seeds(ensemble_seeds(s, 4).reshape(-1), 9).reshape(3, 4, 9))
    assert np.array_equal(t[:, 0, 0], s)                                       # the slice's own seed
    e = ensemble_seeds(s, 4)
    for k in range(4):
        assert np.array_equal(t[:, k, :], tile_seeds(e[:, k], 9))             # a replica is an ordinary sample_tiled call
    assert np.array_equal(t[:, :, 0], e)
    assert np.array_equal(t[:, 0, :], tile_seeds(s, 9))                        # K = 1 is sample_tiled of the slice
    assert np.array_equal(tiled_ensemble_seeds(s, 1, 1), np.array(s).reshape(3, 1, 1))
    assert int(t.min()) >= 0 and int(t.max()) < 2 ** 62
    # a tensor of seeds is taken like a list
    import torch
    assert np.array_equal(tiled_ensemble_seeds(torch.tensor(s, dtype=torch.int64), 4, 9), t)


def test_composed_seeds_are_distinct():
    from founddiff_amd.tiling import tiled_ensemble_seeds
    seeds = np.concatenate([np.arange(4096, dtype=np.int64), np.arange(2 ** 62 - 64, 2 ** 62, dtype=np.int64)])
    t = tiled_ensemble_seeds(seeds, 16, 16)
    assert t.shape == (4160, 16, 16) and t.size == 1064960
    assert int(t.min()) >= 0 and int(t.max()) < 2 ** 62
    assert len(np.unique(t)) == t.size


def test_seed_errors():
    from founddiff_amd.tiling import tiled_ensemble_seeds
    with pytest.raises(RuntimeError, match="K must be at least 1"):
        tiled_ensemble_seeds([1], 0, 4)
    with pytest.raises(RuntimeError, match="n_tiles must be at least 1"):
        tiled_ensemble_seeds([1], 2, 0)
    for bad in (-1, 2 ** 62):
        with pytest.raises(RuntimeError, match="outside"):
            tiled_ensemble_seeds([5, bad], 2, 4)


def test_cabi_declares_the_entry_point():
    from founddiff_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "founddiff_hip.h")).read()
    assert "int " + ENTRY + "(" in hdr
    assert len(L.SIGNATURES[ENTRY][1]) == 20
    for build in (L.BF16, L.F16):
        assert hasattr(build.lib(), ENTRY)


def test_entry_rejects_bad_arguments_without_launching():
    """null pointers other than `samples`, K < 1 and fd_tiles.hip's shape limits fail in the entry itself, with a message"""
    from founddiff_amd import _lib as L
    one = 16                                                             # never dereferenced: every call fails its checks first
    ok = (1, 2, 8, 8, 8, 8, 1, 1, 1)                                     # B, K, H, W, th, tw, my, mx, xs_mult4
    for build in (L.BF16, L.F16):
        lib = build.lib()
        call = lambda ptrs, shape: lib.fd_tiles_ensemble_f32(*ptrs, *shape, None)
        ptrs = [one] * 10
        for i in range(10):
            if i == 5:                                                   # samples may be NULL: that call is checked on the GPU
                continue
            p = list(ptrs)
            p[i] = None
            assert call(p, ok) != 0 and b"fd_tiles_ensemble_f32: null pointer" in lib.fd_last_error(), i
        for K in (0, -3):
            assert call(ptrs, (1, K, 8, 8, 8, 8, 1, 1, 1)) != 0 and b"K must be at least 1" in lib.fd_last_error()
        for B, K, H, W, th, tw, my, mx in ((1, 1, 8, 8, 9, 8, 1, 1), (1, 1, 8, 8, 8, 9, 1, 1), (1, 1, 8, 8, 8, 8, 0, 1),
                                           (1, 1, 8, 8, 8, 8, 1, 0), (65536, 1, 8, 8, 8, 8, 1, 1), (8192, 1, 8, 8, 8, 8, 4, 2),
                                           (1, 65536, 8, 8, 8, 8, 1, 1), (16, 512, 8, 8, 8, 8, 4, 2), (1, 1, 32769, 8, 8, 8, 1, 1),
                                           (1, 1, 8, 32769, 8, 8, 1, 1), (0, 1, 8, 8, 8, 8, 1, 1), (1, 1, 8, 8, 0, 8, 1, 1)):
            assert call(ptrs, (B, K, H, W, th, tw, my, mx, 1)) != 0
            assert b"fd_tiles_ensemble_f32: unsupported shape" in lib.fd_last_error(), (B, K, H, W, th, tw, my, mx)


@pytest.mark.parametrize("half", ["bf16", "fp16"])
def test_kernels_use_no_scratch_and_no_agprs(half):
    from founddiff_amd import build
    tab = build.resources(half).get("fd_tiles_ensemble.hip")
    assert tab, "no resource report for fd_tiles_ensemble.hip"
    mine = {k: v for k, v in tab.items() if "tiles_ensemble" in k}
    # the 16-byte form, the scalar form and the finish kernel
    assert len([k for k in mine if "tiles_ensemble_kernelILb1" in k]) == 1
    assert len([k for k in mine if "tiles_ensemble_kernelILb0" in k]) == 1
    assert len([k for k in mine if "tiles_ensemble_finish_kernel" in k]) == 1
    for name, r in tab.items():                                          # and the partial sum this file instantiates
        assert r["scratch"] == 0 and r["agpr"] == 0, (name, r)


def test_public_interface():
    from founddiff_amd import parallel
    from founddiff_amd.DADiff import ResidualDiffusion, Trainer
    p = inspect.signature(ResidualDiffusion.sample_ensemble).parameters
    assert list(p)[:5] == ["self", "x_input", "n_samples", "slice_seeds", "return_samples"]
    for name, default in (("tile", None), ("overlap", 0), ("tile_condition", "tile"), ("tile_fuse", "final")):
        assert p[name].kind is inspect.Parameter.KEYWORD_ONLY and p[name].default == default, name
    assert inspect.signature(Trainer.test).parameters["tiled_ensemble"].default is False
    assert inspect.signature(parallel.sample_volume).parameters["tiled_ensemble"].default is False


def test_arguments_are_checked_before_any_work():
    """the host-side checks of sample_ensemble(tile=...) need no device"""
    from founddiff_amd.DADiff import ResidualDiffusion

    class _Stub:
        input_condition = False
        _sample_ensemble_tiled = ResidualDiffusion._sample_ensemble_tiled
        _tiled_args = ResidualDiffusion._tiled_args
    run = ResidualDiffusion.sample_ensemble.__wrapped__
    with pytest.raises(RuntimeError, match="n_samples must be at least 1"):
        run(_Stub(), [None], 0, tile=32)
    with pytest.raises(RuntimeError, match="tile_fuse must be 'final' or 'step'"):
        run(_Stub(), [None], 2, tile=32, tile_fuse="each")
    with pytest.raises(RuntimeError, match="condition must be 'tile' or 'slice'"):
        run(_Stub(), [None], 2, tile=32, tile_condition="row")
    with pytest.raises(RuntimeError, match="tile must be an int or a pair"):
        run(_Stub(), [None], 2, tile=2.5)
    with pytest.raises(RuntimeError, match=r"x_input must be \[ldct"):
        run(_Stub(), [None], 2, tile=32)
    with pytest.raises(TypeError):                                       # keyword-only
        run(_Stub(), [None], 2, None, False, 32)
    _Stub.input_condition = True
    with pytest.raises(RuntimeError, match="input_condition"):
        run(_Stub(), [None], 2, tile=32)


def test_callers_raise_without_the_switch():
    """tile with n_samples > 1 is opt-in on both callers; the message names the switch"""
    from founddiff_amd import parallel
    from founddiff_amd.DADiff import Trainer
    import torch

    class _Dif:
        def parameters(self):
            return iter([torch.zeros(1)])
    with pytest.raises(RuntimeError, match="ensembles of tiled samples.*tiled_ensemble=True"):
        parallel.sample_volume(_Dif(), torch.zeros(2, 1, 8, 8), tile=8, n_samples=2)
    with pytest.raises(RuntimeError, match="ensembles of tiled samples.*tiled_ensemble=True"):
        Trainer.test.__wrapped__(object(), tile=8, n_samples=2)
