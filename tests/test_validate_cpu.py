"""Validation during training (founddiff_amd.diffusion_train.val_draws / val_items / val_summary, ResidualDiffusion.eval_items,
Trainer(val_dataset=..., validate_every=...), csrc/fd_validate.hip), host side, without a GPU: the draws as a pure function, the
per-band summary against numpy, the error paths that need no GPU, the C ABI of both builds and the resources of the new kernels."""
import inspect
import os
import re
import shutil

import numpy as np
import pytest
import torch

from test_train_data_cpu import _raises

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("fd_val_items_ws_floats", "fd_val_items_f32")
BANDS = (0, 250, 500, 750, 1000)


def test_val_draws_is_a_pure_function_keyed_per_item_and_band():
    from founddiff_amd.diffusion_train import _mix64, val_draws
    idx = [7, 2, 9, 40]
    item, band, t, seeds = val_draws(5, idx, BANDS, 1000)
    for a in (item, band, t, seeds):
        assert a.dtype == np.int64 and a.shape == (16,)
    assert item.tolist() == [i for i in idx for _ in range(4)] and band.tolist() == [0, 1, 2, 3] * 4       # items outer, bands inner
    lo, hi = np.asarray(BANDS)[band], np.asarray(BANDS)[band + 1]
    assert ((t >= lo) & (t < hi)).all()
    assert (seeds >= 0).all() and (seeds < 1 << 62).all()
    assert t.tolist() == [BANDS[k] + _mix64(5, i, k, 0x76) % 250 for i in idx for k in range(4)]
    assert seeds.tolist() == [_mix64(5, i, k, 0x6E) >> 2 for i in idx for k in range(4)]
    again = val_draws(5, idx, BANDS, 1000)
    assert all(np.array_equal(a, b) for a, b in zip((item, band, t, seeds), again))
    # an item's (t, seed) does not depend on what else is evaluated, or in which order
    of = lambda res, i: [(int(tt), int(ss)) for ii, tt, ss in zip(res[0], res[2], res[3]) if ii == i]
    for other in ([9, 7], [40, 1, 2, 3, 7, 9, 100], [7]):
        res = val_draws(5, other, BANDS, 1000)
        for i in set(other) & set(idx):
            assert of(res, i) == of((item, band, t, seeds), i), (other, i)
    # the seed and the band both key the draw
    many = list(range(64))
    base = val_draws(5, many, BANDS, 1000)
    moved = val_draws(6, many, BANDS, 1000)
    assert (moved[2] != base[2]).any() and (moved[3] != base[3]).all()
    off4, s4 = base[2].reshape(64, 4) - np.asarray(BANDS[:4]), base[3].reshape(64, 4)
    assert (off4[:, 0] != off4[:, 1]).any()                             # not one offset reused in every band
    assert len(set(base[3].tolist())) == 256 and (s4[:, 0] != s4[:, 1]).all()
    # bands of unequal widths, the last one ending at T; a band of one timestep
    _, _, tu, _ = val_draws(5, many, (0, 1, 10, 1000), 1000)
    tu = tu.reshape(64, 3)
    assert (tu[:, 0] == 0).all() and ((tu[:, 1] >= 1) & (tu[:, 1] < 10)).all() and ((tu[:, 2] >= 10) & (tu[:, 2] < 1000)).all()
    assert set(tu[:, 1].tolist()) == set(range(1, 10))                  # 64 draws out of 9 values: every one is met
    assert all(a.shape == (0,) for a in val_draws(5, [], BANDS, 1000))


def test_val_draws_known_answers():
    """three (val_seed, item) pairs, all four bands each: the numbers a log of any run of any version can be compared by"""
    from founddiff_amd.diffusion_train import val_draws
    known = {(0, 0): ([244, 455, 507, 967],
                      [4331840844586797199, 1636339787125472887, 3812585007160951505, 1699646448829892596]),
             (7, 3): ([66, 391, 743, 928],
                      [1470954002661200291, 2657668030736648558, 1586640281527632691, 3914320919683125077]),
             (123456789, 4095): ([84, 302, 565, 770],
                                 [2397397061060486578, 4068395111902373698, 3036758942646127070, 4273472749690059035])}
    for (seed, i), (t, s) in known.items():
        item, band, got_t, got_s = val_draws(seed, [i], BANDS, 1000)
        assert item.tolist() == [i] * 4 and band.tolist() == [0, 1, 2, 3]
        assert got_t.tolist() == t and got_s.tolist() == s, (seed, i)


def test_bad_band_edges_raise():
    from founddiff_amd.diffusion_train import check_bands, val_draws
    for bad in ((0, 500, 500, 1000), (0, 600, 500, 1000), (-1, 500, 1000), (0, 500, 1001), (1000, 0)):
        _raises("must increase strictly inside", val_draws, 0, [0], bad, 1000)
    for bad in ((0,), (), 1000, None, (0, 500.0, 1000), (0, True)):
        _raises("bands must be a tuple", val_draws, 0, [0], bad, 1000)
    assert check_bands("x", [0, np.int64(3), 1000], 1000) == (0, 3, 1000)
    assert check_bands("x", (999, 1000), 1000) == (999, 1000)


def test_val_summary_against_numpy():
    """float64 sums of at most a few hundred float32 values: rel 1e-12 is float64's rounding with room to spare"""
    from founddiff_amd.diffusion_train import val_summary
    rng = np.random.default_rng(3)
    n, nb = 300, 5
    items = np.stack([rng.random(n) * 0.3, rng.random(n) * 1e-2 + 1e-6], axis=1).astype(np.float32)
    band = rng.integers(0, nb - 1, n)                                   # band 4 stays empty
    items[band == 2, 1] = np.nan                                        # ... and band 2 has no residual output
    got = val_summary(items, band, nb)
    assert sorted(got) == ["loss", "mse", "n", "psnr", "rmse"] and all(len(v) == nb for v in got.values())
    x = items.astype(np.float64)
    for k in range(nb):
        rows = x[band == k]
        assert got["n"][k] == len(rows)
        if k == 4:
            assert len(rows) == 0 and all(np.isnan(got[c][k]) for c in ("loss", "mse", "psnr", "rmse"))
            continue
        assert abs(got["loss"][k] - rows[:, 0].mean()) <= 1e-12 * rows[:, 0].mean()
        if k == 2:
            assert all(np.isnan(got[c][k]) for c in ("mse", "psnr", "rmse"))
            continue
        want = {"mse": rows[:, 1].mean(), "psnr": (-10 * np.log10(rows[:, 1])).mean(), "rmse": np.sqrt(rows[:, 1]).mean()}
        for c, w in want.items():
            assert abs(got[c][k] - w) <= 1e-12 * abs(w), (c, k)
        # the mean of the per-item PSNRs, not the PSNR of the mean MSE
        assert abs(got["psnr"][k] + 10 * np.log10(got["mse"][k])) > 1e-3
    assert sum(got["n"]) == n
    one = val_summary(items[:1], band[:1], nb)
    assert one["n"][int(band[0])] == 1 and one["loss"][int(band[0])] == float(items[0, 0])
    none = val_summary(np.zeros((0, 2), np.float32), np.zeros(0, np.int64), 2)
    assert none["n"] == [0, 0] and np.isnan(none["loss"]).all()
    exact = val_summary(np.asarray([[0.5, 0.0]], np.float32), np.asarray([0]), 1)      # a perfect item: infinite PSNR, no warning
    assert exact["psnr"] == [float("inf")] and exact["rmse"] == [0.0]
    _raises("inconsistent shapes", val_summary, items[:, :1], band, nb)
    _raises("inconsistent shapes", val_summary, items, band[:-1], nb)
    _raises("inconsistent shapes", val_summary, items, band.astype(np.float64), nb)
    _raises("band 3 outside", val_summary, items, band, 3)


def test_val_items_rejects_before_cuda_is_initialised():
    """types and dtypes, then shapes, then devices, each with its message, and nothing touches the GPU"""
    from founddiff_amd import diffusion_train as dt
    was = torch.cuda.is_initialized()
    a, b = torch.zeros(2, 1, 4, 4), torch.zeros(2, 1, 4, 4)
    _raises("pred must be a tensor", dt.val_items, None, b, "l1")
    _raises("target must be float32", dt.val_items, a, b.double(), "l1")
    _raises("x_start must be float32", dt.val_items, a, b, "l1", a, b.half())
    _raises("invalid loss type", dt.val_items, a, b, "huber")
    _raises("both x_input and x_start", dt.val_items, a, b, "l1", a)
    _raises("both x_input and x_start", dt.val_items, a, b, "l1", None, a)
    _raises("inconsistent shapes", dt.val_items, a, b[:1], "l1")
    _raises("inconsistent shapes", dt.val_items, a, b, "l2", a, b[:, :, :2])
    _raises("inconsistent shapes", dt.val_items, torch.zeros(0, 4), torch.zeros(0, 4), "l1")
    _raises("no CPU path", dt.val_items, a, b, "l1")
    _raises("no CPU path", dt.val_items, a, b, "l2", a, b)
    assert torch.cuda.is_initialized() == was


def _tiny(num_unet=1, objective="pred_res"):
    from founddiff_amd.DADiff import ResidualDiffusion, UnetRes
    net = UnetRes(64, dim_mults=(1, 2), num_unet=num_unet, condition=True, objective=objective,
                  clip_cfg=dict(layers=(1, 1, 1, 1), width=16, embed_dim=1024))
    return ResidualDiffusion(net, image_size=64, objective=objective, condition=True)


def test_trainer_validation_arguments(tmp_path):
    from founddiff_amd.DADiff import Trainer
    from founddiff_amd.data import SyntheticCTDataset
    was = torch.cuda.is_initialized()
    sig = inspect.signature(Trainer.__init__).parameters
    defaults = dict(val_dataset=None, validate_every=0, val_bands=(0, 250, 500, 750, 1000), val_items=None, val_seed=0,
                    val_batch_size=8, keep_best=False)
    for name, d in defaults.items():
        assert sig[name].default == d and sig[name].kind is inspect.Parameter.KEYWORD_ONLY, name
    assert list(sig)[-len(defaults):] == list(defaults)                 # after everything that was there
    assert all(name in Trainer.__doc__ for name in defaults)
    assert "CHECKPOINT_KEYS" in Trainer.train.__doc__ and "resumed" in Trainer.train.__doc__
    dif, ds = _tiny(), SyntheticCTDataset(3, 64)
    kw = dict(checkpoint_folder=str(tmp_path), device="cpu")
    for bad in ((0, 500, 500, 1000), (0, 600, 500), (-1, 1000), (0, 1001)):
        _raises("must increase strictly inside \\[0, 1000\\]", Trainer, None, dif, val_bands=bad, **kw)
    _raises("bands must be a tuple", Trainer, None, dif, val_bands=(0,), **kw)
    _raises("validate_every=2 needs a val_dataset", Trainer, None, dif, validate_every=2, **kw)
    _raises("invalid validation arguments", Trainer, None, dif, validate_every=-1, **kw)
    _raises("invalid validation arguments", Trainer, None, dif, val_dataset=ds, val_batch_size=0, **kw)
    _raises("invalid validation arguments", Trainer, None, dif, val_dataset=ds, val_items=0, **kw)
    _raises("invalid validation arguments", Trainer, None, dif, val_dataset=ds, val_seed=0.5, **kw)
    tr = Trainer(None, dif, **kw)                                       # everything off by default
    assert tr.validate_every == 0 and tr.val_dataset is None and tr.val_log == [] and tr.best is None and not tr.keep_best
    assert tr.val_bands == (0, 250, 500, 750, 1000)
    _raises("val_dataset", tr.validate)
    tr = Trainer(None, dif, val_dataset=ds, validate_every=1, val_bands=[0, 500, 1000], val_items=2, keep_best=True, **kw)
    assert tr.val_bands == (0, 500, 1000) and tr.val_items == 2 and tr.keep_best
    _raises("no CPU path", tr.validate)
    assert tr.val_log == [] and tr._val_store is None
    # eval_items: forward-only needs no optimiser, so two U-Nets get as far as the tensors' device
    x = torch.zeros(2, 1, 64, 64)
    for model in (dif, _tiny(2, "pred_res_noise")):
        _raises("no CPU path", model.eval_items, [x, x], torch.tensor([3, 999]))
        _raises("imgs must be", model.eval_items, x, torch.tensor([3, 999]))
        _raises("t must be int64", model.eval_items, [x, x], torch.tensor([3.0, 999.0]))
        assert model.model.unet0._trainable is None and not any(p.requires_grad for p in model.parameters())
    assert torch.cuda.is_initialized() == was


def test_val_score_picks_psnr_where_there_is_a_residual_output():
    from founddiff_amd.DADiff import Trainer
    nan = float("nan")
    res = {"n": [2, 2], "loss": [[0.1, 0.3], [0.5, 0.7]], "psnr": [[30.0, 20.0], [nan, nan]]}
    assert Trainer._val_score(res) == ("psnr", 25.0)
    metric, value = Trainer._val_score(dict(res, psnr=[[nan, nan], [nan, nan]]))
    assert metric == "loss" and abs(value - 0.4) < 1e-15


def test_new_entries_are_declared_and_exported():
    """declared in include/founddiff_hip.h, present in _lib's table, exported by both builds of the library"""
    from founddiff_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "founddiff_hip.h")).read()
    assert re.search(r"\bint64_t fd_val_items_ws_floats\(", hdr) and re.search(r"\bint fd_val_items_f32\(", hdr)
    assert len(L.SIGNATURES["fd_val_items_f32"][1]) == 10 and L.SIGNATURES["fd_val_items_ws_floats"][0] is L.i64
    for build in (L.BF16, L.F16):
        lib = build.lib()
        for name in NEW_SYMBOLS:
            assert hasattr(lib, name), name


def test_entry_rejects_bad_arguments_without_launching():
    """null pointers, one of x_input / x_start alone, an unknown loss type and shapes outside fd_res_loss_f32's limits fail in
    the entry itself, with a message, before any launch; the workspace follows the loss's rule with two columns"""
    from founddiff_amd import _lib as L
    one = 16                                                             # never dereferenced: every call fails its checks first
    for build in (L.BF16, L.F16):
        lib = build.lib()
        for B, npix in ((2, 512 * 512), (1, 1), (5, 8193), (65535, 4)):
            n = lib.fd_val_items_ws_floats(B, npix)
            chunks = (npix + 8191) // 8192
            assert n == ((2 * B * chunks + 3) & ~3) + ((2 * B * ((chunks + 31) // 32) + 3) & ~3), (B, npix, n)
            assert n >= 2 * lib.fd_res_loss_ws_floats(B, npix) - 8
        bad_shapes = ((0, 16), (65536, 16), (2, 0), (2, -4), (2, 1 << 40))
        for B, npix in bad_shapes:
            assert lib.fd_val_items_ws_floats(B, npix) == 0 and lib.fd_res_loss_ws_floats(B, npix) == 0
            assert lib.fd_val_items_f32(one, one, None, None, 1, one, one, B, npix, None) != 0
            assert b"fd_val_items_f32: unsupported shape" in lib.fd_last_error(), (B, npix)
        for args in ((None, one, None, None, 1, one, one), (one, None, None, None, 1, one, one), (one, one, None, None, 1, None, one),
                     (one, one, one, one, 2, one, None)):
            assert lib.fd_val_items_f32(*args, 2, 16, None) != 0
            assert b"fd_val_items_f32: null pointer" in lib.fd_last_error()
        for xi, x0 in ((one, None), (None, one)):
            assert lib.fd_val_items_f32(one, one, xi, x0, 1, one, one, 2, 16, None) != 0
            assert b"both x_input and x_start" in lib.fd_last_error()
        for lt in (0, 3):
            assert lib.fd_val_items_f32(one, one, one, one, lt, one, one, 2, 16, None) != 0
            assert b"loss_type must be 1 (l1) or 2 (l2)" in lib.fd_last_error()


def test_new_kernels_use_no_scratch():
    """0 bytes of scratch per lane for the eight instantiations of val_items_kernel (16-byte / scalar x l1 / l2 x with / without
    the denoising column) and for the finish, in both builds; one or two 256-float arrays of LDS for the workgroup sums"""
    if not shutil.which("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    from founddiff_amd import build
    for half in ("bf16", "fp16"):
        build.build(half=half)
        tab = build.resources(half).get("fd_validate.hip")
        assert tab, "no resource remarks beside fd_validate.hip's object: rebuild with build(force=True)"
        main = {name: r for name, r in tab.items() if "val_items_kernel" in name}
        assert len(main) == 8 and any("val_finish_kernel" in name for name in tab), sorted(tab)
        for name, r in tab.items():
            assert r.get("scratch", 0) == 0, (half, name, r)
        for name, r in main.items():
            assert r.get("lds", 0) == (2048 if "Lb1EEEv" in name else 1024), (half, name, r)         # the last flag: DENOISE
