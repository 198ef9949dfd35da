"""Validation during training on the GPU: fd_val_items_f32 (csrc/fd_validate.hip) against float64 numpy, ResidualDiffusion.eval_items
on the tiny model of tests/test_gpu_own_train.py against its float64 reference and against the training path, Trainer.validate
(batching, repeatability, the numbers follow the weights), validation inside train() leaves the run bit for bit alone, keep_best.

Gates: OUT = 1e-5 of tests/test_gpu_train_step.py / test_gpu_own_train.py for forward outputs, rel = |a - b| / |b| per number."""
import functools
import os

import numpy as np
import pytest
import torch

from test_gpu_own_train import DIM, MULTS, OUT, SIZE, T, TINY_CLIP, _batch, _diffusion, _reference, _state, _trainer

pytestmark = pytest.mark.gpu
# (B, npix): one pixel; a scalar tail alone; one 16-byte chunk of a workgroup's 8192; npix % 4 != 0 (the scalar form); exactly half a
# chunk; nine chunks with a ragged last one, more than one workgroup per slice
SHAPES = [(1, 1), (2, 5), (3, 1024), (2, 4097), (5, 4096), (2, 70001)]
BANDS2 = (0, 500, 1000)


def _inputs(B, npix, seed, offset=0):
    """pred = 1.5 randn, so that both clamps act; target = randn; x_input, x_start uniform in [-1, 1]; where there is room, entries
    exactly on the clamps: pred = +-1, x_input - clamp(pred) = +-1 and beyond, x_start = +-1.  offset: every tensor starts that
    many floats past a 16-byte boundary."""
    g = torch.Generator().manual_seed(seed)
    n = B * npix
    pred, target = 1.5 * torch.randn(n, generator=g), torch.randn(n, generator=g)
    x_input, x_start = 2 * torch.rand(n, generator=g) - 1, 2 * torch.rand(n, generator=g) - 1
    if n >= 8:
        k = torch.randperm(n, generator=g)[:8]
        pred[k[0]], pred[k[1]] = 1.0, -1.0
        pred[k[2]], x_input[k[2]] = -1.0, 0.0                            # x0_hat = 1 exactly
        pred[k[3]], x_input[k[3]] = 1.0, 0.0                             # ... and -1
        pred[k[4]], x_input[k[4]] = -3.0, 0.5                            # 1.5, clamped
        x_start[k[5]], x_start[k[6]] = 1.0, -1.0
        pred[k[7]], target[k[7]] = 0.25, 0.25                            # a zero difference
    out = []
    for v in (pred, target, x_input, x_start):
        buf = torch.empty(n + 4, device="cuda")
        w = buf[offset:offset + n]
        w.copy_(v)
        assert w.data_ptr() % 16 == 4 * offset
        out.append(w.view(B, npix))
    return out


def _items_f64(pred, target, x_input, x_start, loss_type):
    """the issue's formulas in float64 numpy, from the float32 inputs"""
    p, q, xi, x0 = (v.detach().cpu().double().numpy() for v in (pred, target, x_input, x_start))
    d = p - q
    col0 = (np.abs(d) if loss_type == "l1" else d * d).mean(axis=1)
    u = lambda v: np.clip((v + 1) / 2, 0, 1)
    hat = np.clip(xi - np.clip(p, -1, 1), -1, 1)
    col1 = ((u(hat) - u(x0)) ** 2).mean(axis=1)
    return np.stack([col0, col1], axis=1)


def _worst(got, want):
    return float((np.abs(got.double().cpu().numpy() - want) / np.abs(want)).max())


@pytest.mark.parametrize("loss_type", ["l1", "l2"])
@pytest.mark.parametrize("B,npix", SHAPES)
def test_val_items_against_float64(B, npix, loss_type):
    from founddiff_amd.diffusion_train import val_items
    pred, target, x_input, x_start = _inputs(B, npix, seed=1000 * B + npix)
    want = _items_f64(pred, target, x_input, x_start, loss_type)
    got = val_items(pred, target, loss_type, x_input, x_start)
    assert got.shape == (B, 2) and got.dtype == torch.float32 and got.is_cuda and not got.requires_grad
    err = _worst(got, want)
    print(f"[measured] val_items {loss_type} B={B} npix={npix}: worst rel {err:.2e} (gate {OUT:.0e})")
    assert err < OUT, (err, got.cpu(), want)
    assert torch.equal(got, val_items(pred, target, loss_type, x_input, x_start))          # two runs, the same bits
    # without the images: the same loss column, NaN beside it
    bare = val_items(pred, target, loss_type)
    assert torch.equal(bare[:, 0], got[:, 0]) and bool(torch.isnan(bare[:, 1]).all())
    # (B, 1, H, W) where npix factors, and a prediction that asks for gradients: nothing is differentiable
    if npix % 4 == 0:
        shaped = [v.view(B, 1, 4, npix // 4) for v in (pred, target, x_input, x_start)]
        assert torch.equal(val_items(shaped[0].clone().requires_grad_(), shaped[1], loss_type, *shaped[2:]), got)


def test_val_items_off_the_16_byte_boundary():
    """every pointer one float past a 16-byte boundary takes the scalar form: against float64, and the bits of the 16-byte form"""
    from founddiff_amd.diffusion_train import val_items
    B, npix = 5, 4096
    for loss_type in ("l1", "l2"):
        off = _inputs(B, npix, seed=77, offset=1)
        want = _items_f64(*off, loss_type)
        got = val_items(off[0], off[1], loss_type, off[2], off[3])
        err = _worst(got, want)
        print(f"[measured] val_items {loss_type} off the boundary: worst rel {err:.2e}")
        assert err < OUT, err
        on = _inputs(B, npix, seed=77)
        assert torch.equal(got, val_items(on[0], on[1], loss_type, on[2], on[3]))


def test_val_items_rows_do_not_depend_on_the_batch():
    from founddiff_amd.diffusion_train import val_items
    for npix in (4096, 70001):
        pred, target, x_input, x_start = _inputs(5, npix, seed=5)
        full = val_items(pred, target, "l1", x_input, x_start)
        for b in range(5):
            alone = val_items(*(v[b:b + 1].clone() for v in (pred, target)), "l1", *(v[b:b + 1].clone() for v in (x_input, x_start)))
            assert torch.equal(alone[0], full[b]), (npix, b)


def test_val_items_rejects_one_image_alone():
    from founddiff_amd import _lib as L
    from founddiff_amd._train import ptr, stream, workspace
    from founddiff_amd.diffusion_train import val_items
    pred, target, x_input, x_start = _inputs(2, 16, seed=9)
    with pytest.raises(RuntimeError, match="both x_input and x_start"):
        val_items(pred, target, "l1", x_input=x_input)
    with pytest.raises(RuntimeError, match="both x_input and x_start"):
        val_items(pred, target, "l1", x_start=x_start)
    # ... and the entry itself, handed live pointers
    items, ws = torch.empty(2, 2, device="cuda"), workspace("fd_val_items_ws_floats", pred.device, 2, 16)
    with pytest.raises(L.FoundDiffHipError, match="both x_input and x_start"):
        L.call("fd_val_items_f32", ptr(pred), ptr(target), ptr(x_input), None, 1, ptr(items), ptr(ws), 2, 16, stream(pred.device))
    with pytest.raises(RuntimeError, match="x_input must live on the GPU"):
        val_items(pred, target, "l1", x_input.cpu(), x_start)


# ---- eval_items on the tiny model ----------------------------------------------------------------------------------------------
def test_eval_items_against_the_float64_reference_and_the_training_path():
    from founddiff_amd import diffusion_train as dt
    from founddiff_amd.data import DeviceSliceStore
    from oracle import metrics
    ref_loss, _ = _reference("pred_res", "l1")
    dif = _diffusion("pred_res", "l1")
    x_start, x_input, t, noise = (v.cuda() for v in _batch())
    out = dif.eval_items([x_start, x_input], t, noise=noise)
    assert isinstance(out, list) and len(out) == 1
    items = out[0]
    assert items.shape == (2, 2) and items.is_cuda and not items.requires_grad
    # forward-only: no trainable view, no parameter asks for a gradient
    assert dif.model.unet0._trainable is None and not any(p.requires_grad for p in dif.parameters())
    got = float(items[:, 0].double().mean())
    e_ref = abs(got - ref_loss) / abs(ref_loss)
    trained = _diffusion("pred_res", "l1")
    loss = float(trained([x_start, x_input], t=t, noise=noise)[0].detach().double())
    e_train = abs(got - loss) / abs(loss)
    print(f"[measured] eval_items pred_res l1: mean of column 0 {got:.8f}, float64 {ref_loss:.8f} rel {e_ref:.2e}, the training "
          f"path {loss:.8f} rel {e_train:.2e}")
    assert e_ref < OUT, e_ref
    assert e_train < OUT, e_train
    # column 1 from the engine's own output, in float64
    sch = dict(alphas_cumsum=dif.alphas_cumsum, betas_cumsum=dif.betas_cumsum)
    x_in, x_res, _, times, x0 = dt.q_sample(x_start, x_input, t, sch, noise=noise, x0_out=True)
    x_t, xi = x_in[:, 0:1].contiguous(), x_in[:, 1:2].contiguous()
    eng = dif.model.unet0.engine("fp32")
    eng.encode_condition(xi)
    pred = eng.forward(x_t, xi, times[0]).clone()
    assert torch.equal(dt.val_items(pred, x_res, "l1", xi, x0), items)                      # what eval_items composes
    u = lambda v: ((v.double().cpu() + 1) / 2).clamp(0, 1)
    hat = (xi.double().cpu() - pred.double().cpu().clamp(-1, 1)).clamp(-1, 1)
    mse = torch.stack([metrics.rmse(u(hat)[b], u(x0)[b]) ** 2 for b in range(2)])
    psnr = torch.stack([metrics.psnr(u(hat)[b], u(x0)[b]) for b in range(2)])
    e_mse = float(((items[:, 1].double().cpu() - mse).abs() / mse).max())
    print(f"[measured] eval_items column 1: one-step MSE {items[:, 1].tolist()} (PSNR {psnr.tolist()} dB at t = {t.tolist()}), "
          f"rel {e_mse:.2e} to float64 from the engine's output")
    assert e_mse < OUT, e_mse
    # a StoreBatch of the same pair, and keyed noise: a list of tensors and the store give the same bits
    store = DeviceSliceStore.from_items([[x_start[b].cpu(), x_input[b].cpu()] for b in range(2)], "cuda")
    seeds = torch.tensor([11, 12], device="cuda")
    a = dif.eval_items([x_start, x_input], t, slice_seeds=seeds, step=3)[0]
    b = dif.eval_items(dt.StoreBatch(store, [0, 1]), t.cpu().numpy(), slice_seeds=seeds.cpu().numpy(), step=3)[0]
    assert torch.equal(a, b) and not torch.equal(a, items)
    assert dif.model.unet0._trainable is None and not any(p.requires_grad for p in dif.parameters())


@functools.lru_cache(maxsize=None)
def _weights2():
    from founddiff_amd import arch, synth
    w = {}
    for u, seed in (("unet0", 0), ("unet1", 1)):
        w.update(synth.synth_state_dict(arch.da_unet_spec(DIM, MULTS, prefix=f"model.{u}.", clip=TINY_CLIP), seed=seed))
    return w


def test_eval_items_two_unets_and_the_sampling_precision():
    from founddiff_amd.DADiff import ResidualDiffusion, UnetRes, load_weights
    x_start, x_input, t, noise = (v.cuda() for v in _batch())
    net = UnetRes(dim=DIM, dim_mults=MULTS, num_unet=2, condition=True, objective="pred_res_noise", test_res_or_noise="res_noise",
                  precision="fp32", clip_cfg=TINY_CLIP)
    two = ResidualDiffusion(net, image_size=SIZE, timesteps=T, sampling_timesteps=2, objective="pred_res_noise", loss_type="l2",
                            condition=True, sum_scale=0.01, test_res_or_noise="res_noise")
    load_weights(two, _weights2(), "synthetic weights")
    two = two.to("cuda")
    out = two.eval_items([x_start, x_input], t, noise=noise)
    assert len(out) == 2 and all(o.shape == (2, 2) for o in out)
    assert bool(torch.isfinite(out[0]).all()) and bool(torch.isfinite(out[1][:, 0]).all()) and bool(torch.isnan(out[1][:, 1]).all())
    assert two.model.unet0._trainable is None and not any(p.requires_grad for p in two.parameters())
    with pytest.raises(NotImplementedError):                             # training two U-Nets stays unbuilt
        two([x_start, x_input], t=t, noise=noise)
    # unet0 of the pair has unet0's weights of the one-U-Net model and the same routing (times[0], x_res): the same bits, l2 here
    one = _diffusion("pred_res", "l2")
    assert torch.equal(one.eval_items([x_start, x_input], t, noise=noise)[0], out[0])
    # precision=None: the model's sampling precision, bf16
    half = _diffusion("pred_res", "l1", precision="bf16")
    lo = half.eval_items([x_start, x_input], t, noise=noise, precision=None)[0]
    hi = half.eval_items([x_start, x_input], t, noise=noise)[0]
    assert ("bf16", 0) in half.model.unet0._engine and ("fp32", 0) in half.model.unet0._engine
    gap = float(((lo - hi).abs() / hi.abs()).max())
    print(f"[measured] eval_items on the bf16 engine against the fp32 engine: worst rel {gap:.2e}; fp32 {hi.tolist()} bf16 {lo.tolist()}")
    assert bool(torch.isfinite(lo).all()) and np.isfinite(gap)
    assert torch.equal(hi, _diffusion("pred_res", "l1").eval_items([x_start, x_input], t, noise=noise)[0])


# ---- Trainer.validate ----------------------------------------------------------------------------------------------------------
def _val_trainer(folder, steps, **kw):
    from founddiff_amd.data import SyntheticCTDataset
    args = dict(val_dataset=SyntheticCTDataset(6, SIZE, seed=11), val_bands=BANDS2, save_and_sample_every=100)
    args.update(kw)
    return _trainer(folder, steps, **args)


def _numbers(res):
    return np.asarray([res[k] for k in ("loss", "psnr", "rmse")], dtype=np.float64)


def test_validate(tmp_path):
    tr = _val_trainer(tmp_path, 2, val_batch_size=2)
    r2 = tr.validate()
    assert sorted(r2) == ["bands", "loss", "n", "psnr", "rmse", "step"]
    assert r2["step"] == 0 and r2["bands"] == [0, 500, 1000] and r2["n"] == [6, 6]
    assert _numbers(r2).shape == (3, 1, 2) and np.isfinite(_numbers(r2)).all()            # per U-Net, then per band
    assert tr.ema.ema_model is tr.model and tr.model.model.unet0._trainable is None        # nothing was set up for training
    assert r2 == tr.validate() and len(tr.val_log) == 2 and tr.val_log[0] is r2            # two calls in a row: the same bits
    tr.val_batch_size = 5                                                # 12 (item, band) pairs: 5 + 5 + 2
    r5 = tr.validate()
    gap = float((np.abs(_numbers(r5) - _numbers(r2)) / np.abs(_numbers(r2))).max())
    print(f"[measured] validate(): batches of 2 against 5: worst rel {gap:.2e}, bitwise equal: {r5 == r2}; loss {r2['loss'][0]}, "
          f"one-step psnr {r2['psnr'][0]}, rmse {r2['rmse'][0]}")
    assert gap < OUT, gap
    # the first items only; another seed moves the numbers
    tr.val_items = 4
    assert tr.validate()["n"] == [4, 4]
    tr.val_items, tr.val_seed = None, 1
    assert tr.validate()["loss"] != r5["loss"]
    tr.val_seed = 0
    # after train() has moved the weights (the EMA copy follows at once here), the numbers change, and stay repeatable
    tr.train()
    assert tr.step == 2 and tr.ema.ema_model is not tr.model and tr._stale
    after = tr.validate()
    assert not tr._stale and after["step"] == 2 and after["n"] == [6, 6]
    assert after["loss"] != r5["loss"] and after["psnr"] != r5["psnr"]
    assert {k: v for k, v in tr.validate().items()} == after
    print(f"[measured] validate() after 2 steps: loss {after['loss'][0]} (before: {r5['loss'][0]})")


def test_validation_does_not_disturb_training(tmp_path):
    with_val = _val_trainer(tmp_path / "a", 4, validate_every=1)
    without = _val_trainer(tmp_path / "b", 4, validate_every=0)
    with_val.train()
    without.train()
    sa, ca = _state(with_val)
    sb, cb = _state(without)
    assert ca == cb and with_val.batch_log == without.batch_log
    bad = [k for k in sa if not torch.equal(sa[k], sb[k])]
    assert sorted(sa) == sorted(sb) and not bad, bad[:5]
    assert [r["step"] for r in with_val.val_log] == [1, 2, 3, 4] and without.val_log == []
    first, last = with_val.val_log[0], with_val.val_log[-1]
    print(f"[measured] validate_every=1 over 4 steps: band losses {first['loss'][0]} -> {last['loss'][0]}, one-step psnr "
          f"{first['psnr'][0]} -> {last['psnr'][0]}")
    assert all(np.isfinite(_numbers(r)).all() for r in with_val.val_log)


def test_keep_best(tmp_path):
    from founddiff_amd.DADiff import Trainer
    from founddiff_amd.diffusion_train import CHECKPOINT_KEYS
    tr = _val_trainer(tmp_path, 1, validate_every=1, keep_best=True)
    path = os.path.join(tr.results_folder, "model-best.pt")
    assert not os.path.exists(path)
    tr.train()
    assert os.path.exists(path) and tr.best["step"] == 1 and tr.best["metric"] == "psnr"
    data = torch.load(path, map_location="cpu", weights_only=False)
    assert sorted(data) == sorted(CHECKPOINT_KEYS) and data["step"] == 1
    tr.train_num_steps = 3
    tr.train()
    scores = {r["step"]: Trainer._val_score(r)[1] for r in tr.val_log}
    assert sorted(scores) == [1, 2, 3] and tr.best["step"] in scores
    assert scores[tr.best["step"]] == max(scores.values()) == tr.best["value"]
    print(f"[measured] keep_best: mean one-step psnr per step {scores}, best {tr.best}")
    data = torch.load(path, map_location="cpu", weights_only=False)
    assert sorted(data) == sorted(CHECKPOINT_KEYS) and data["step"] == tr.best["step"]
    other = _val_trainer(tmp_path, 3)
    other.load("best")
    assert other.step == tr.best["step"]
    resumed = _val_trainer(tmp_path, 3)
    resumed.load("best", for_training=True)
    assert resumed.step == tr.best["step"] and resumed.val_log == [] and resumed.best is None
