"""The structural loss term without a GPU: the reference of tests/ssim_loss_ref.py against the pinned oracle, the closed-form
gradient (the formula and border fold csrc/fd_ssim_train.hip implements) against float64 autograd, the new keywords' defaults,
what raises before anything launches, and val_summary's third column."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import ssim_loss_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("fd_ssim_loss_ws_floats", "fd_ssim_loss_f32", "fd_onestep_u01_f32")


def _raises(match, fn, *args, **kw):
    with pytest.raises(RuntimeError, match=match):
        fn(*args, **kw)


@pytest.mark.parametrize("shape", R.SHAPES)
def test_reference_is_the_oracle_ssim(shape):
    """the float64 reference's clamped map, averaged per slice, is oracle/metrics.py's SSIM of that slice (float32, 2-D window)"""
    from oracle import metrics as om
    for residual in (True, False):
        out, x_start, x_input = R.make_inputs(shape, residual)
        p, y = R.images(out.double(), x_start.double(), None if x_input is None else x_input.double(), residual)
        m = R.ssim_map(p, y)
        assert float(m.min()) < 1.0 and float(m.max()) <= 1.0 + 1e-12
        for b in range(shape[0]):
            want = float(om.ssim(p[b:b + 1].float(), y[b:b + 1].float()))
            got = float(m[b].clamp(0, 1).mean())
            assert abs(got - want) < 2e-5, (shape, residual, b, got, want)       # the oracle's float32 composition: its own error


def test_the_map_goes_below_zero_on_the_recipe():
    """why the loss does not clamp: on the recipe's inputs S < 0 occurs"""
    lo = []
    for shape in R.SHAPES:
        out, x_start, x_input = (v.double() for v in R.make_inputs(shape, True))
        lo.append(float(R.ssim_map(*R.images(out, x_start, x_input, True)).min()))
    assert min(lo) < 0.0, lo


@pytest.mark.parametrize("residual", (True, False))
@pytest.mark.parametrize("shape", R.SHAPES)
def test_closed_form_gradient_against_autograd(shape, residual):
    """the formulas of include/founddiff_hip.h with the adjoint's border fold equal float64 autograd of the composition to 1e-12
    of max|g|, in the value, the items and the gradient, for both row kinds and under a scale"""
    inp = R.make_inputs(shape, residual)
    for scale in (1.0, 0.37):
        t64, i64, g64 = R.reference(*inp, residual, scale)
        t, items, g = R.closed_form(*inp, residual, scale)
        assert abs(t - float(t64)) < 1e-13 and np.abs(items - i64.numpy()).max() < 1e-13
        err = np.abs(g - g64.numpy()).max() / float(g64.abs().max())
        assert err < 1e-12, (shape, residual, scale, err)


def test_double_fold_on_short_axes():
    """n in 6 .. 10: both folds land on one j; the adjoint of the reflect-padded filter is the transpose of its matrix"""
    g = R.window().numpy()
    for n in range(6, 14):
        M = np.zeros((n, n))
        for i in range(n):
            for d in range(-5, 6):
                k = i + d
                k = -k if k < 0 else (2 * (n - 1) - k if k >= n else k)
                M[i, k] += g[d + 5]
        c = np.random.default_rng(n).standard_normal((3, n))
        assert np.abs(R.adjoint_axis(c, -1) - c @ M).max() < 1e-14, n


def test_signature_defaults():
    from founddiff_amd import diffusion_train as dt
    from founddiff_amd.DADiff import ResidualDiffusion, Trainer
    sig = inspect.signature
    p = sig(dt.p_losses_fn).parameters
    assert list(p)[-1] == "ssim_weight" and p["ssim_weight"].default == 0.0
    assert sig(dt.train_step).parameters["ssim_weight"].default == 0.0
    p = sig(dt.structural_loss).parameters
    assert list(p) == ["out", "x_start", "x_input", "residual", "scale"] and p["x_input"].default is None and p["scale"].default == 1.0
    assert p["residual"].kind is inspect.Parameter.KEYWORD_ONLY and p["residual"].default is inspect.Parameter.empty
    assert list(sig(dt.ssim_items).parameters) == ["out", "x_start", "x_input", "residual"]
    p = sig(ResidualDiffusion.__init__).parameters
    assert list(p)[-1] == "ssim_weight" and p["ssim_weight"].default == 0.0 and p["ssim_weight"].kind is inspect.Parameter.KEYWORD_ONLY
    p = sig(ResidualDiffusion.eval_items).parameters
    assert list(p) == ["self", "imgs", "t", "noise", "slice_seeds", "step", "precision", "ssim"] and p["ssim"].default is False
    assert p["precision"].default == "fp32"
    p = sig(Trainer.__init__).parameters
    for name, d in (("ssim_weight", None), ("val_ssim", False)):
        assert p[name].default is d and p[name].kind is inspect.Parameter.KEYWORD_ONLY, name
    assert list(sig(Trainer.validate).parameters) == ["self", "precision"]
    assert "ssim_weight" in Trainer.__doc__ and "val_ssim" in Trainer.__doc__ and "resumed run must be given it again" in Trainer.__doc__


def _tiny(num_unet=1, objective="pred_res", **kw):
    from founddiff_amd.DADiff import ResidualDiffusion, UnetRes
    net = UnetRes(64, dim_mults=(1, 2), num_unet=num_unet, condition=True, objective=objective,
                  clip_cfg=dict(layers=(1, 1, 1, 1), width=16, embed_dim=1024))
    return ResidualDiffusion(net, image_size=64, objective=objective, condition=True, **kw)


def test_what_raises_before_anything_launches(tmp_path):
    from founddiff_amd import diffusion_train as dt
    from founddiff_amd.DADiff import Trainer, residual_schedule
    was = torch.cuda.is_initialized()
    x, t = torch.zeros(2, 1, 64, 64), torch.tensor([3, 999])
    sched = residual_schedule(1000)
    never = lambda *a: pytest.fail("the model was called")
    for bad in (-0.5, float("nan"), float("inf"), "1", None, True):
        _raises("ssim_weight must be a finite number >= 0", dt.p_losses_fn, never, [x, x], t, sched, ssim_weight=bad)
    _raises("ssim_weight must be a finite number", _tiny, ssim_weight=-1.0)
    _raises("ssim_weight must be a finite number", Trainer, None, _tiny(), ssim_weight=float("nan"), checkpoint_folder=str(tmp_path),
            device="cpu")
    # an objective without a one-step estimate, named
    _raises("'pred_noise' predicts the noise alone", dt.p_losses_fn, never, [x, x], t, sched, objective="pred_noise", ssim_weight=0.5)
    dif = _tiny(1, "pred_noise", ssim_weight=0.25)
    _raises("'pred_noise' predicts the noise alone", dt.p_losses, dif, [x, x], t)
    # H or W < 6: reflect padding of 5
    small = torch.zeros(2, 1, 5, 64)
    _raises("needs H, W >= 6", dt.p_losses_fn, never, [small, small], t, sched, ssim_weight=0.5)
    _raises("needs H, W >= 6", dt.structural_loss, small, small, small, residual=True)
    _raises("needs H, W >= 6", dt.ssim_items, torch.zeros(1, 64, 5), torch.zeros(1, 64, 5), residual=False)
    _raises("needs crops of at least 6 x 6", Trainer, None, _tiny(), ssim_weight=0.5, crop_size=(2, 64), checkpoint_folder=str(tmp_path),
            device="cpu")
    # the other checks of structural_loss, in _check_loss's order: types, shapes, devices
    _raises("needs x_input", dt.structural_loss, x, x, residual=True)
    _raises("residual must be a bool", dt.structural_loss, x, x, x, residual=1)
    _raises("out must be float32", dt.structural_loss, x.double(), x, residual=False)
    _raises("scale must be a number", dt.structural_loss, x, x, residual=False, scale="1")
    _raises("inconsistent shapes", dt.structural_loss, x, x[:1], residual=False)
    _raises("inconsistent shapes", dt.structural_loss, torch.zeros(2, 2, 64, 64), torch.zeros(2, 2, 64, 64), residual=False)
    _raises("no CPU path", dt.structural_loss, x, x, residual=False)
    _raises("no CPU path", dt.ssim_items, x, x, x, residual=True)
    # a Trainer's number lands on the model; None leaves the model's own
    tr = Trainer(None, _tiny(), ssim_weight=0.5, val_ssim=True, checkpoint_folder=str(tmp_path), device="cpu")
    assert tr.model.ssim_weight == 0.5 and tr.val_ssim and tr.ema.ema_model.ssim_weight == 0.5
    tr = Trainer(None, _tiny(ssim_weight=0.125), checkpoint_folder=str(tmp_path), device="cpu")
    assert tr.model.ssim_weight == 0.125 and tr.ssim_weight is None and not tr.val_ssim
    assert _tiny().ssim_weight == 0.0
    assert torch.cuda.is_initialized() == was


def test_reference_shaped_objects_have_no_term():
    """_diffusion_args reads the attribute through getattr: an object without it trains as before"""
    from founddiff_amd import diffusion_train as dt
    dif = _tiny()
    assert dt._diffusion_args("p_losses", dif)[-1] == 0.0
    del dif.ssim_weight
    assert dt._diffusion_args("p_losses", dif)[-1] == 0.0
    dif.ssim_weight = 0.5
    assert dt._diffusion_args("p_losses", dif)[-1] == 0.5


def test_val_summary_third_column():
    from founddiff_amd.diffusion_train import val_summary
    rng = np.random.default_rng(3)
    items = np.concatenate([rng.random((7, 2)) * 0.01 + 1e-4, rng.random((7, 1))], 1).astype(np.float32)
    band = np.asarray([0, 1, 0, 1, 1, 0, 1])
    got, two = val_summary(items, band, 2), val_summary(items[:, :2], band, 2)
    assert list(two) == ["loss", "mse", "psnr", "rmse", "n"] and list(got) == ["loss", "mse", "psnr", "rmse", "ssim", "n"]
    assert all(got[k] == two[k] for k in two)
    for k in range(2):
        assert abs(got["ssim"][k] - items[band == k, 2].astype(np.float64).mean()) < 1e-15
    nan = items.copy()
    nan[:, 2] = np.nan
    assert all(np.isnan(v) for v in val_summary(nan, band, 2)["ssim"])
    assert np.isnan(val_summary(np.zeros((0, 3), np.float32), np.zeros(0, np.int64), 1)["ssim"][0])
    _raises("inconsistent shapes", val_summary, np.zeros((7, 4), np.float32), band, 2)


def test_new_entries_are_declared_and_exported():
    """declared in include/founddiff_hip.h, present in _lib's table, exported by both builds of the library; the host-side
    refusals of the entry points need no GPU"""
    import ctypes as C
    from founddiff_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "founddiff_hip.h")).read()
    assert re.search(r"\bint64_t fd_ssim_loss_ws_floats\(", hdr) and re.search(r"\bint fd_ssim_loss_f32\(", hdr)
    assert re.search(r"\bint fd_onestep_u01_f32\(", hdr)
    assert all(name in L.SIGNATURES for name in NEW_SYMBOLS)
    one = C.c_void_p(C.addressof((C.c_float * 4)()))
    for build in (L.BF16, L.F16):
        lib = build.lib()
        for B, H, W in ((2, 512, 512), (1, 6, 6), (3, 17, 33)):
            n = lib.fd_ssim_loss_ws_floats(B, H, W)
            assert n >= 3 * B * H * W + B * -(-H // 16) * -(-W // 16) + B and n % 4 == 0
        for B, H, W in ((0, 64, 64), (65536, 64, 64), (1, 5, 64), (1, 64, 5)):
            assert lib.fd_ssim_loss_ws_floats(B, H, W) == 0
        assert lib.fd_ssim_loss_f32(one, one, 36, one, 1, 1.0, one, one, one, 0, one, 1, 5, 6, None) != 0
        assert b"H, W >= 6" in lib.fd_last_error()
        assert lib.fd_ssim_loss_f32(one, one, 36, one, 1, 1.0, one, one, one, 0, one, 65536, 6, 6, None) != 0
        assert b"at most 65535 slices" in lib.fd_last_error()
        assert lib.fd_ssim_loss_f32(one, None, 0, one, 1, 1.0, one, one, one, 0, one, 1, 6, 6, None) != 0
        assert b"needs x_input" in lib.fd_last_error()
        assert lib.fd_ssim_loss_f32(one, one, 36, one, 1, 1.0, one, one, one, 0, None, 1, 6, 6, None) != 0
        assert b"null pointer" in lib.fd_last_error()
        assert lib.fd_onestep_u01_f32(one, one, 16, one, one, None, 1, 16, None) != 0
        assert b"null pointer" in lib.fd_last_error()
        assert lib.fd_onestep_u01_f32(one, one, 8, one, one, one, 1, 16, None) != 0
        assert b"unsupported shape" in lib.fd_last_error()
