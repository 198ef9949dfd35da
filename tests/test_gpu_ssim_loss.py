"""The structural loss term on the GPU (csrc/fd_ssim_train.hip, founddiff_amd.diffusion_train.structural_loss / ssim_items /
p_losses_fn(ssim_weight=...), Trainer(ssim_weight=..., val_ssim=...)) against the float64 composition of tests/ssim_loss_ref.py.

Gates: 4 x the worst error, over the shape list and both row kinds, of the SAME composition run in float32 on the CPU against
float64 on the same inputs (ssim_loss_ref.gates(), computed when the tests run): absolute in the value and the items,
max|g - g64| / max|g64| in the gradient.  Everything about repeatability is bitwise."""
import numpy as np
import pytest
import torch

import ssim_loss_ref as R
from test_gpu_own_train import SIZE, _diffusion, _state, _trainer

pytestmark = pytest.mark.gpu
KINDS = (True, False)                 # a residual row, an x0 row
DEGENERATE = (2, 17, 33)


def _cuda(inp):
    return tuple(None if v is None else v.cuda() for v in inp)


def _run(inp, residual, scale=1.0):
    """(term, items, gradient) of the kernels, on the CPU"""
    from founddiff_amd import diffusion_train as dt
    out, x_start, x_input = _cuda(inp)
    out.requires_grad_(True)
    term = dt.structural_loss(out, x_start, x_input, residual=residual, scale=scale)
    assert term.shape == () and term.requires_grad and term.dtype == torch.float32
    term.backward()
    items = dt.ssim_items(out, x_start, x_input, residual=residual)
    assert items.shape == (out.shape[0],) and not items.requires_grad
    return term.detach().cpu(), items.cpu(), out.grad.cpu()


@pytest.mark.parametrize("residual", KINDS)
@pytest.mark.parametrize("shape", R.SHAPES)
def test_against_float64(shape, residual):
    gv, gi, gg = R.gates()
    inp, (t64, i64, g64), (t32, i32, g32) = R.case(shape, residual)
    term, items, grad = _run(inp, residual)
    ev, ei, eg = abs(float(term) - float(t64)), float((items.double() - i64).abs().max()), R.grad_err(grad, g64)
    print(f"[measured] structural_loss {shape} residual={residual}: value {float(term):.8f} err {ev:.2e} (gate {gv:.2e}; float32 "
          f"composition {abs(float(t32) - float(t64)):.2e}), items err {ei:.2e} (gate {gi:.2e}), gradient err {eg:.2e} (gate {gg:.2e}; "
          f"float32 composition {R.grad_err(g32, g64):.2e})")
    assert ev <= gv and ei <= gi and eg <= gg, (ev, gv, ei, gi, eg, gg)
    # the value is the items' mean, in double, rounded once
    assert float(term) == float(np.float32(1.0 - items.double().mean().item()))


@pytest.mark.parametrize("residual", KINDS)
def test_scale_reaches_value_and_gradient(residual):
    gv, _, gg = R.gates()
    inp = R.make_inputs((2, 7, 23), residual)
    t64, _, g64 = R.reference(*inp, residual, scale=0.37)
    term, _, grad = _run(inp, residual, scale=0.37)
    assert abs(float(term) - float(t64)) <= gv and R.grad_err(grad, g64) <= gg


@pytest.mark.parametrize("residual", KINDS)
def test_degenerate_inputs(residual):
    """p == y: the value is 0 within the value gate and max|g| stays below the gradient gate x max|g64| of the noisy case at the
    same shape.  Constant images against float64: with zero variance the three adjoint terms are each of the order 1 / C2 and
    cancel to a gradient of order 1, so the error floor is an absolute one, eps / C2; its scale is therefore the larger of
    max|g64| of the constant case and of the noisy case, the scale the p == y check has."""
    gv, gi, gg = R.gates()
    _, (_, _, g64_noisy), _ = R.case(DEGENERATE, residual)
    B, H, W = DEGENERATE
    # p == y bit for bit: x0 row out = x_start; residual row x_input = x_start, out = 0
    _, x_start, _ = R.make_inputs(DEGENERATE, residual)
    inp = (torch.zeros_like(x_start), x_start, x_start.clone()) if residual else (x_start.clone(), x_start, None)
    term, items, grad = _run(inp, residual)
    worst = float(grad.abs().max())
    print(f"[measured] p == y residual={residual}: value {float(term):.3e} (gate {gv:.2e}), max|g| {worst:.3e} (gate "
          f"{gg * float(g64_noisy.abs().max()):.3e})")
    assert abs(float(term)) <= gv and float((items.double() - 1).abs().max()) <= gi
    assert worst <= gg * float(g64_noisy.abs().max())
    # constant images, zero variance: two different levels against float64, one common level like p == y
    lo, hi = torch.full((B, 1, H, W), -0.4), torch.full((B, 1, H, W), 0.2)
    inp = (hi - lo, hi, hi.clone()) if residual else (lo, hi, None)                      # residual: p = (hi - (hi - lo) + 1) / 2
    t64, i64, g64 = R.reference(*inp, residual)
    term, items, grad = _run(inp, residual)
    assert abs(float(term) - float(t64)) <= gv and float((items.double() - i64).abs().max()) <= gi
    assert float((grad.double() - g64).abs().max()) <= gg * max(float(g64.abs().max()), float(g64_noisy.abs().max()))
    inp = (torch.zeros_like(hi), hi, hi.clone()) if residual else (hi.clone(), hi, None)
    term, _, grad = _run(inp, residual)
    assert abs(float(term)) <= gv and float(grad.abs().max()) <= gg * float(g64_noisy.abs().max())


@pytest.mark.parametrize("residual", KINDS)
def test_bitwise_properties(residual):
    from founddiff_amd import diffusion_train as dt
    shape = (3, 17, 33)
    inp = R.make_inputs(shape, residual)
    a, b = _run(inp, residual), _run(inp, residual)
    assert all(torch.equal(u, v) for u, v in zip(a, b))                                   # two calls, equal bits
    for k in range(3):                                                                    # a slice's item is its batch-1 item
        one = tuple(None if v is None else v[k:k + 1] for v in inp)
        assert torch.equal(_run(one, residual)[1], a[1][k:k + 1]), k
    # the gradient row of a batch of 4 under scale 4 is the batch-1 row under scale 1
    four = R.make_inputs((4, 17, 33), residual, seed=2)
    g4 = _run(four, residual, scale=4.0)[2]
    for k in (0, 3):
        one = tuple(None if v is None else v[k:k + 1] for v in four)
        assert torch.equal(_run(one, residual, scale=1.0)[2], g4[k:k + 1]), k
    # a strided x_input (a channel of q_sample's x_in) is read where it lies: the bits of its dense copy
    if residual:
        out, x_start, x_input = _cuda(inp)
        pair = torch.stack([torch.zeros_like(x_input[:, 0]), x_input[:, 0]], 1)
        assert torch.equal(dt.ssim_items(out, x_start, pair[:, 1:2], residual=True).cpu(), a[1])


def _model_fn(outs):
    return lambda x_in, times: list(outs)


@pytest.mark.parametrize("objective", ("pred_res", "pred_x0_noise", "pred_res_noise"))
def test_p_losses_is_the_sum_of_the_two_terms(objective):
    """p_losses_fn(ssim_weight=w) = residual_loss + structural_loss(scale = scale w), in the loss and in out.grad, bit for bit;
    the noise row is residual_loss alone; ssim_weight=0.0 is the call without the keyword"""
    from founddiff_amd import diffusion_train as dt
    from founddiff_amd import objectives
    from founddiff_amd.DADiff import residual_schedule
    rows = objectives.TRAINING[objective]
    B, H, W = 2, 17, 33
    g = torch.Generator().manual_seed(5)
    x_start, x_input = ((torch.rand(B, 1, H, W, generator=g) * 2 - 1).cuda() for _ in range(2))
    noise, t = torch.randn(B, 1, H, W, generator=g).cuda(), torch.tensor([700, 20]).cuda()
    outs = [torch.randn(B, 1, H, W, generator=g).cuda() * 0.3 for _ in rows]
    sched, scale, w = residual_schedule(1000), 0.5, 0.75
    for loss_type in ("l1", "l2"):
        got = [o.clone().requires_grad_(True) for o in outs]
        losses = dt.p_losses_fn(_model_fn(got), [x_start, x_input], t, sched, objective, loss_type, noise=noise, scale=scale, ssim_weight=w)
        assert len(losses) == len(rows)
        for loss in losses:
            loss.backward()
        x_in, x_res, nz, _ = dt.q_sample(x_start, x_input, t, sched, noise=noise, normalize=False)
        targets = {"res": x_res, "noise": nz, "x0": x_start}
        for r, o, loss, have in zip(rows, outs, losses, got):
            want = o.clone().requires_grad_(True)
            total = dt.residual_loss(want, targets[r.target], loss_type, scale)
            if r.target != "noise":
                total = total + dt.structural_loss(want, x_start, x_input if r.residual else None, residual=r.residual, scale=scale * w)
            total.backward()
            assert torch.equal(loss.detach(), total.detach()), (objective, loss_type, r)
            assert torch.equal(have.grad, want.grad), (objective, loss_type, r)
        plain = [o.clone().requires_grad_(True) for o in outs]
        zero = [o.clone().requires_grad_(True) for o in outs]
        la = dt.p_losses_fn(_model_fn(plain), [x_start, x_input], t, sched, objective, loss_type, noise=noise, scale=scale)
        lb = dt.p_losses_fn(_model_fn(zero), [x_start, x_input], t, sched, objective, loss_type, noise=noise, scale=scale, ssim_weight=0.0)
        for u, v in zip(la + lb, plain + zero):
            u.backward()
        assert all(torch.equal(u, v) for u, v in zip(la, lb)) and all(torch.equal(u.grad, v.grad) for u, v in zip(plain, zero))
    with pytest.raises(RuntimeError, match="'pred_noise' predicts the noise alone"):
        dt.p_losses_fn(_model_fn(outs[:1]), [x_start, x_input], t, sched, "pred_noise", ssim_weight=w)


def _grads(dif, batch):
    x_start, x_input, t, noise = batch
    losses = dif([x_start, x_input], t=t, noise=noise)
    for loss in losses:
        loss.backward()
    grads = {k: p.grad.clone() for k, p in dif.named_parameters() if p.grad is not None}
    dif.zero_grad(set_to_none=True)
    return [v.detach().clone() for v in losses], grads


def test_weight_zero_is_a_model_without_the_attribute():
    from test_gpu_own_train import _batch
    batch = tuple(v.cuda() for v in _batch())
    dif = _diffusion()
    assert dif.ssim_weight == 0.0
    l0, g0 = _grads(dif, batch)
    del dif.ssim_weight                                   # a reference-shaped object
    l1, g1 = _grads(dif, batch)
    assert g0 and sorted(g0) == sorted(g1)
    assert all(torch.equal(u, v) for u, v in zip(l0, l1)) and all(torch.equal(g0[k], g1[k]) for k in g0)
    dif.ssim_weight = 0.5                                 # and the term moves both
    l2, g2 = _grads(dif, batch)
    assert float(l2[0]) > float(l0[0]) and any(not torch.equal(g0[k], g2[k]) for k in g0)


# ---- the whole path ------------------------------------------------------------------------------------------------------------
def _run_trainer(folder, steps, **kw):
    args = dict(save_and_sample_every=100, gradient_accumulate_every=1, log_every=1, ssim_weight=0.5)
    args.update(kw)
    tr = _trainer(folder, steps, **args)
    tr.train()
    return tr


def _three_way(tmp_path, make, **kw):
    """A against A' (the same run again) and against B (2 steps, save, a new Trainer, load, 2 steps): every parameter, EMA and
    optimiser tensor and every counter, bit for bit.  Returns A."""
    a, a2 = _run_trainer(tmp_path / "a", 4, dif=make(), **kw), _run_trainer(tmp_path / "a2", 4, dif=make(), **kw)
    (sa, ca), (sa2, ca2) = _state(a), _state(a2)
    assert ca == ca2 and not [k for k in sa if not torch.equal(sa[k], sa2[k])]
    assert a.loss_log == a2.loss_log and a.model.ssim_weight == 0.5 and a.ema.ema_model.ssim_weight == 0.5
    b = _run_trainer(tmp_path / "b", 2, dif=make(), **kw)
    b.save(1)
    b2 = _trainer(tmp_path / "b", 4, dif=make(), save_and_sample_every=100, gradient_accumulate_every=1, log_every=1, ssim_weight=0.5, **kw)
    b2.load(1, for_training=True)
    b2.train()
    sb, cb = _state(b2)
    assert cb == ca and b.batch_log + b2.batch_log == a.batch_log
    bad = [k for k in sa if not torch.equal(sa[k], sb[k])]
    assert not bad, bad[:5]
    assert b.loss_log + b2.loss_log == a.loss_log
    return a


def test_train_repeat_resume_and_the_logged_loss(tmp_path):
    from founddiff_amd import diffusion_train as dt
    a = _three_way(tmp_path, _diffusion)
    assert [s for s, _ in a.loss_log] == [1, 2, 3, 4] and all(np.isfinite(v[0]) for _, v in a.loss_log)
    # step 1's logged loss is residual_loss + structural_loss(scale = 0.5) on the untrained model's output for that micro-batch
    dif, ds = _diffusion(), a.train_dataset
    idx = dt.train_batch_indices(a.seed, 0, 0, a.batch_size, len(ds), 1)
    assert idx == a.batch_log[0]
    t, seeds = dt.train_t_and_seeds(a.seed, 0, 0, idx, dif.num_timesteps)
    items = [ds[i] for i in idx]
    x_start, x_input = (torch.stack([it[j] for it in items]).float().cuda() for j in range(2))
    sched = dict(alphas_cumsum=dif.alphas_cumsum, betas_cumsum=dif.betas_cumsum)
    x_in, x_res, _, times, x0 = dt.q_sample(x_start, x_input, torch.from_numpy(t).cuda(), sched, slice_seeds=torch.from_numpy(seeds).cuda(),
                                            step=0, x0_out=True)
    dif.model.trainable()
    out, = dif.model(x_in, [times[0], times[1]])
    want = dt.residual_loss(out, x_res, "l1", 1.0) + dt.structural_loss(out, x0, x_in[:, 1:2], residual=True, scale=0.5)
    plain = float(dt.residual_loss(out, x_res, "l1", 1.0).detach())
    print(f"[measured] Trainer(ssim_weight=0.5) step 1: loss {a.loss_log[0][1][0]:.8f}, the composition {float(want.detach()):.8f}, l1 alone {plain:.8f}")
    assert a.loss_log[0][1][0] == float(want.detach()) and float(want.detach()) > plain


def test_train_repeat_resume_radam_x0_row(tmp_path):
    from test_gpu_two_unet_train import _two
    a = _three_way(tmp_path, lambda: _two("pred_x0_noise"), optimizer="radam")
    assert len(a.loss_log[0][1]) == 2 and all(np.isfinite(v).all() for _, v in a.loss_log)
    # the x0 row carries the term: the same run without it logs another unet0 loss and the same unet1 loss at step 1
    off = _run_trainer(tmp_path / "off", 1, dif=_two("pred_x0_noise"), optimizer="radam", ssim_weight=None)
    assert off.model.ssim_weight == 0.0
    assert a.loss_log[0][1][0] > off.loss_log[0][1][0] and a.loss_log[0][1][1] == off.loss_log[0][1][1]


def test_validate_with_ssim(tmp_path):
    from founddiff_amd import diffusion_train as dt
    from founddiff_amd.data import SyntheticCTDataset
    from founddiff_amd.metrics import compute_metrics
    bands = (0, 500, 1000)
    kw = dict(val_dataset=SyntheticCTDataset(4, SIZE, seed=11), val_bands=bands, save_and_sample_every=100, val_batch_size=8)     # one batch: 4 items x 2 bands
    off, on = _trainer(tmp_path / "off", 2, **kw), _trainer(tmp_path / "on", 2, val_ssim=True, **kw)
    r0, r1 = off.validate(), on.validate()
    assert sorted(r0) == ["bands", "loss", "n", "psnr", "rmse", "step"] and sorted(r1) == sorted(list(r0) + ["ssim"])
    assert all(r0[k] == r1[k] for k in r0)
    assert np.asarray(r1["ssim"]).shape == (1, 2) and all(0.0 < v <= 1.0 for v in r1["ssim"][0])
    # the composition: q_sample, the engine's output, the one-step estimate in torch ops, compute_metrics
    dif, store = on.ema.ema_model, on._val_store
    item, band, t, seeds = dt.val_draws(on.val_seed, range(4), bands, dif.num_timesteps)
    sched = dict(alphas_cumsum=dif.alphas_cumsum, betas_cumsum=dif.betas_cumsum)
    x_in, _, _, times, x0 = dt.q_sample(dt.StoreBatch(store, item), None, t, sched, slice_seeds=seeds, x0_out=True)
    x_t, xi = x_in[:, 0:1].contiguous(), x_in[:, 1:2].contiguous()
    eng = dif.model.unet0.engine("fp32")
    eng.encode_condition(xi)
    pred = eng.forward(x_t, xi, times[0]).clone()
    est = (((xi - pred.clamp(-1, 1)).clamp(-1, 1) + 1) / 2).clamp(0, 1)
    tgt = ((x0 + 1) / 2).clamp(0, 1)
    e2, t2 = dt.onestep_pair(pred, xi, x0)
    assert torch.equal(e2, est) and torch.equal(t2, tgt)
    col = compute_metrics(est, tgt)[:, 1].cpu().numpy().astype(np.float64)
    for k in range(2):
        v = col[band == k]
        assert r1["ssim"][0][k] == float(v.sum() / v.size), (k, r1["ssim"][0][k], float(v.sum() / v.size))
    # eval_items: (B, 2) by default, (B, 3) with ssim=True, the first two columns untouched; NaN where there is no residual
    two = dif.eval_items(dt.StoreBatch(store, item), t, slice_seeds=seeds)[0]
    three = dif.eval_items(dt.StoreBatch(store, item), t, slice_seeds=seeds, ssim=True)[0]
    assert two.shape == (8, 2) and three.shape == (8, 3) and torch.equal(three[:, :2], two)
    assert np.array_equal(three[:, 2].cpu().numpy().astype(np.float64), col)
    sl = slice(0, 3)
    noise_model = _diffusion("pred_noise")
    out = noise_model.eval_items(dt.StoreBatch(store, item[sl]), t[sl], slice_seeds=seeds[sl], ssim=True)[0]
    assert out.shape == (3, 3) and bool(torch.isnan(out[:, 1:]).all()) and bool(torch.isfinite(out[:, 0]).all())
    print(f"[measured] validate(val_ssim=True): one-step SSIM per band {r1['ssim'][0]}, PSNR {r1['psnr'][0]}")
