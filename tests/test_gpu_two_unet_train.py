"""Training two U-Nets on the project's own classes: UnetRes(num_unet=2) of Unet(64, (1, 2), clip_cfg=TINY_CLIP) with synthetic
weights (another seed per U-Net) on 64 x 64 phantoms, batch 2, as tests/test_gpu_own_train.py builds them.

Gradients by identity, not by a new float64 reference: under 'pred_res_noise' unet0 computes what the one-U-Net 'pred_res' model
with its weights computes and unet1 what the one-U-Net 'pred_noise' model computes, and tests/test_gpu_own_train.py pins both of
those to float64.  The kernels are deterministic and a slice's result does not depend on its batch, so the comparison is bitwise.
Then the joint clip of one diffusion_train.ClipRAdamEMA over both U-Nets, and Trainer(optimizer="radam"): repeat, resume across
RAdam's threshold, the checkpoint with 'opt0' and 'opt1', sample() and validate(); one U-Net with RAdam; the defaults."""
import functools
import os

import pytest
import torch

from conftest import rel_err
from test_gpu_own_train import DIM, MULTS, SIZE, T, TINY_CLIP, _batch, _diffusion, _state, _trainer, _weights

pytestmark = pytest.mark.gpu
P0, P1 = "model.unet0.", "model.unet1."


@functools.lru_cache(maxsize=None)
def _weights2():
    """unet0: the weights of tests/test_gpu_own_train.py's model; unet1: seed 1"""
    from founddiff_amd import arch, synth
    w = dict(_weights())
    w.update(synth.synth_state_dict(arch.da_unet_spec(DIM, MULTS, prefix=P1, clip=TINY_CLIP), seed=1))
    return w


def _unet1_alone():
    """unet1's weights under the names of a one-U-Net model"""
    return {P0 + k[len(P1):]: v for k, v in _weights2().items() if k.startswith(P1)}


def _two(objective="pred_res_noise"):
    from founddiff_amd.DADiff import ResidualDiffusion, UnetRes, load_weights
    net = UnetRes(dim=DIM, dim_mults=MULTS, num_unet=2, condition=True, objective=objective, test_res_or_noise="res_noise",
                  precision="fp32", clip_cfg=TINY_CLIP)
    dif = ResidualDiffusion(net, image_size=SIZE, timesteps=T, sampling_timesteps=2, objective=objective, loss_type="l1",
                            condition=True, sum_scale=0.01, test_res_or_noise="res_noise")
    load_weights(dif, _weights2(), "synthetic weights")
    return dif.to("cuda")


def _trunk_grads(unet):
    return {k: (None if p.grad is None else p.grad.clone()) for k, p in unet.named_parameters() if not k.startswith("dose_encoder.")}


@functools.lru_cache(maxsize=None)
def _one_unet_grads(objective):
    """(loss, {trunk key: gradient}) of the one-U-Net model: 'pred_res' with unet0's weights, 'pred_noise' with unet1's.
    Computed once; nobody writes to it."""
    dif = _diffusion(objective, "l1", weights=None if objective == "pred_res" else _unet1_alone())
    x_start, x_input, t, noise = (v.cuda() for v in _batch())
    losses = dif([x_start, x_input], t=t, noise=noise)
    assert len(losses) == 1
    losses[0].backward()
    return losses[0].detach().clone(), _trunk_grads(dif.model.unet0)


@functools.lru_cache(maxsize=None)
def _two_unet_grads(objective):
    dif = _two(objective)
    x_start, x_input, t, noise = (v.cuda() for v in _batch())
    with pytest.raises(NotImplementedError, match="RAdam"):             # the default: not before the opt-in
        dif([x_start, x_input], t=t, noise=noise)
    views = dif.model.trainable()
    assert len(views) == 2
    losses = dif([x_start, x_input], t=t, noise=noise)
    assert isinstance(losses, list) and len(losses) == 2 and all(v.shape == () and v.requires_grad for v in losses)
    for loss in losses:
        loss.backward()
    frozen = [p for u in (dif.model.unet0, dif.model.unet1) for k, p in u.named_parameters() if k.startswith("dose_encoder.")]
    assert frozen and all(p.grad is None and not p.requires_grad for p in frozen)
    return dif, [v.detach().clone() for v in losses], _trunk_grads(dif.model.unet0), _trunk_grads(dif.model.unet1)


def _same(got, want):
    assert sorted(got) == sorted(want)
    bad = [k for k in want if got[k] is None or want[k] is None or not torch.equal(got[k], want[k])]
    return bad


def test_gradients_are_the_one_unet_models():
    """'pred_res_noise': two losses; every trunk gradient of unet0 has the bits of the one-U-Net 'pred_res' model's, every one of
    unet1 those of the 'pred_noise' model's, and so have the losses; the frozen towers have no gradient"""
    _, losses, g0, g1 = _two_unet_grads("pred_res_noise")
    l_res, want0 = _one_unet_grads("pred_res")
    l_noise, want1 = _one_unet_grads("pred_noise")
    print(f"[measured] two U-Nets pred_res_noise: losses {[float(v) for v in losses]}, one-U-Net models {float(l_res)} {float(l_noise)}")
    assert torch.equal(losses[0], l_res) and torch.equal(losses[1], l_noise)
    assert not _same(g0, want0), _same(g0, want0)[:5]
    assert not _same(g1, want1), _same(g1, want1)[:5]
    assert all(bool(g.any()) for g in g0.values()) and all(bool(g.any()) for g in g1.values())


def test_pred_x0_noise():
    """unet1 agrees bitwise with the 'pred_noise' model; unet0's loss (target: the normalised x_start) agrees with eval_items
    column 0's batch mean to 1e-6; its gradients are finite, non-zero and not the 'pred_res_noise' ones"""
    dif, losses, g0, g1 = _two_unet_grads("pred_x0_noise")
    l_noise, want1 = _one_unet_grads("pred_noise")
    assert torch.equal(losses[1], l_noise)
    assert not _same(g1, want1), _same(g1, want1)[:5]
    x_start, x_input, t, noise = (v.cuda() for v in _batch())
    items = dif.eval_items([x_start, x_input], t, noise=noise)
    assert len(items) == 2
    mean0, loss0 = float(items[0][:, 0].double().mean()), float(losses[0].double())
    gap = abs(mean0 - loss0)
    print(f"[measured] pred_x0_noise: unet0's loss {loss0:.8f}, the batch mean of eval_items column 0 {mean0:.8f}, difference "
          f"{gap:.2e} ({gap / abs(loss0):.2e} relative)")
    assert gap <= 1e-6 * min(1.0, abs(loss0)), gap
    _, _, res0, _ = _two_unet_grads("pred_res_noise")
    assert all(g is not None and bool(torch.isfinite(g).all()) and bool(g.any()) for g in g0.values())
    assert all(not torch.equal(g0[k], res0[k]) for k in g0)


def _trainables(dif):
    dif.model.trainable()
    return [p for p in dif.parameters() if p.requires_grad]


def test_joint_clip():
    """one train_step with one ClipRAdamEMA over both U-Nets: its total norm squared is n0^2 + n1^2 of the two one-U-Net steps
    to 1e-6; with max_norm=None the parameters of both U-Nets after the step have the bits of the one-U-Net steps; with
    max_norm=1 the same norm gives the coefficient of clip_grad_norm_"""
    from founddiff_amd.diffusion_train import ClipRAdamEMA, train_step
    x_start, x_input, t, noise = (v.cuda() for v in _batch())
    batch = [x_start, x_input]

    def step(dif, max_norm):
        params = _trainables(dif)
        opt = ClipRAdamEMA(params, lr=1e-3, max_norm=max_norm)
        losses = train_step(dif, opt, batch, t=t, noise=noise)
        return losses, opt._rec.clone(), opt
    one_res, one_noise = _diffusion("pred_res", "l1"), _diffusion("pred_noise", "l1", weights=_unet1_alone())
    (l0,), rec0, _ = step(one_res, None)
    (l1,), rec1, _ = step(one_noise, None)
    two = _two()
    before = {k: v.detach().clone() for k, v in two.state_dict().items()}
    losses, rec, opt = step(two, None)
    assert len(losses) == 2 and torch.equal(losses[0], l0) and torch.equal(losses[1], l1)
    n0, n1, n = float(rec0[0].double()), float(rec1[0].double()), float(rec[0].double())
    e = abs(n * n - (n0 * n0 + n1 * n1)) / (n0 * n0 + n1 * n1)
    print(f"[measured] joint clip: total norm {n:.6f}, one-U-Net norms {n0:.6f} {n1:.6f}, n^2 against n0^2 + n1^2: {e:.2e}")
    assert e < 1e-6, e
    assert float(rec[1]) == 1.0 and float(rec0[1]) == 1.0 and float(rec1[1]) == 1.0
    after = two.state_dict()
    for name, one in ((P0, one_res), (P1, one_noise)):
        want = one.state_dict()
        keys = [k for k in after if k.startswith(name)]
        assert keys
        bad = [k for k in keys if not torch.equal(after[k], want[P0 + k[len(name):]])]
        assert not bad, bad[:5]
        moved = [k for k in keys if ".dose_encoder." not in k and not torch.equal(after[k], before[k])]
        assert moved, name
    assert opt.steps() == [1] * len(opt.params)
    clipped = _two()
    _, rec_c, _ = step(clipped, 1.0)
    assert torch.equal(rec_c[0], rec[0])
    want = min(1.0, 1.0 / (n + 1e-6))
    assert abs(float(rec_c[1]) - want) < 1e-6 * want, (n, float(rec_c[1]), want)


# ---- Trainer(optimizer="radam") ------------------------------------------------------------------------------------------------
def _trainer2(folder, steps, **kw):
    from founddiff_amd.data import SyntheticCTDataset
    args = dict(optimizer="radam", save_and_sample_every=100, val_dataset=SyntheticCTDataset(4, SIZE, seed=11), val_bands=(0, 500, 1000),
                dif=_two())
    args.update(kw)
    return _trainer(folder, steps, **args)          # train_batch_size=2, gradient_accumulate_every=2, ema_update_every=1, lr 1e-3


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """A and A': 8 steps each; B: 4 steps, save, a new Trainer, load(for_training=True), 4 steps.  The resume crosses from RAdam's
    plain steps (1-5) into the rectified ones, so a lost step count shows."""
    root = tmp_path_factory.mktemp("two_unets")
    out = {}
    for name in ("a", "a2"):
        tr = _trainer2(root / name, 8)
        tr.train()
        out[name] = tr
    b = _trainer2(root / "b", 4)
    b.train()
    b.save(1)
    out["saved"], _ = _state(b)
    b2 = _trainer2(root / "b", 8)
    b2.load(1, for_training=True)
    out["loaded"], out["loaded_counters"] = _state(b2)
    b2.train()
    out.update(b=b, b2=b2, folder=root / "b")
    return out


def test_repeat_and_resume(runs):
    a, a2, b, b2 = runs["a"], runs["a2"], runs["b"], runs["b2"]
    from founddiff_amd.diffusion_train import ClipRAdamEMA
    assert isinstance(a.opt0, ClipRAdamEMA) and not hasattr(a, "opt1") and a.opt0.betas == (0.9, 0.999) and a.opt0.max_norm == 1.0
    n_train = len(a.opt0.params)
    assert n_train == sum(1 for p in a.model.parameters() if p.requires_grad) and n_train % 2 == 0
    assert len(a.losses) == 2 and all(bool(torch.isfinite(v).all()) for v in a.losses)
    sa, ca = _state(a)
    sa2, ca2 = _state(a2)
    differ = [k for k in sa if not torch.equal(sa[k], sa2[k])]
    print(f"[measured] two U-Nets, 8 steps: last losses {[float(v) for v in a.losses]}; A against A': {len(differ)} of {len(sa)} "
          f"tensors differ {differ[:3]}")
    assert ca == ca2 == (8, 8, True, [8] * n_train) and a.batch_log == a2.batch_log
    assert not differ, differ[:5]
    saved, loaded = runs["saved"], runs["loaded"]
    assert runs["loaded_counters"] == (4, 4, True, [4] * n_train)      # the round trip itself is bitwise, and the counters
    assert sorted(saved) == sorted(loaded) and all(torch.equal(saved[k], loaded[k]) for k in saved)
    sb, cb = _state(b2)
    assert cb == ca and b.batch_log + b2.batch_log == a.batch_log
    bad = [k for k in sa if not torch.equal(sa[k], sb[k])]
    gap = max(rel_err(sb[k].float(), sa[k].float()) for k in sa if sa[k].is_floating_point() and sa[k].numel())
    print(f"[measured] two U-Nets, resume at step 4 of 8: A against B {gap:.2e}, {len(bad)} tensors differ {bad[:3]}")
    assert not bad, bad[:5]
    # both U-Nets trained, their towers did not
    w = _weights2()
    moved = [k for k, p in a.model.named_parameters() if p.requires_grad and not torch.equal(sa["model." + k], w[k])]
    assert len(moved) == n_train
    assert all(torch.equal(sa["model." + k], w[k]) and torch.equal(sa["ema." + k], w[k]) for k in w if ".dose_encoder." in k)


def test_checkpoint_of_two_unets(runs):
    from founddiff_amd.diffusion_train import CHECKPOINT_KEYS_2
    b = runs["b"]
    data = torch.load(os.path.join(b.results_folder, "model-1.pt"), map_location="cpu", weights_only=False)
    assert sorted(data) == sorted(CHECKPOINT_KEYS_2) and data["scaler"] is None and data["step"] == 4
    place = {id(p): j for j, p in enumerate(b.opt0.params)}
    for entry, unet in (("opt0", b.model.model.unet0), ("opt1", b.model.model.unet1)):
        ps = list(unet.parameters())
        live = [k for k, p in enumerate(ps) if p.requires_grad]
        assert data[entry]["param_groups"][0]["params"] == list(range(len(ps))) and sorted(data[entry]["state"]) == live
        opt = torch.optim.RAdam([torch.nn.Parameter(p.detach().clone()) for p in ps], lr=1.0)
        opt.load_state_dict(data[entry])                                # as torch.optim.RAdam's own
        group = opt.param_groups[0]
        assert group["lr"] == 1e-3 and group["betas"] == (0.9, 0.999) and group["weight_decay"] == 0
        for k in live:
            st = opt.state[opt.param_groups[0]["params"][k]]
            assert float(st["step"]) == 4
            assert torch.equal(st["exp_avg"].cpu(), runs["saved"][f"exp_avg.{place[id(ps[k])]}"])
            assert torch.equal(st["exp_avg_sq"].cpu(), runs["saved"][f"exp_avg_sq.{place[id(ps[k])]}"])
    assert sorted(k for k in data["ema"] if not k.startswith("ema_model.")) == ["initted", "step"] and int(data["ema"]["step"]) == 4
    # a one-U-Net Adam run does not take this file
    one = _trainer(runs["folder"], 4, save_and_sample_every=100, optimizer="adam")
    with pytest.raises(RuntimeError, match="keys"):
        one.load(1, for_training=True)


def test_sample_and_validate_after_training(runs):
    from founddiff_amd import synth
    a = runs["a"]
    x_in = torch.from_numpy(synth.ct_phantom(1, SIZE, seed=12)[1]).cuda()
    noise = torch.randn(1, 1, SIZE, SIZE, generator=torch.Generator().manual_seed(10)).cuda()
    a.sample(9)                                                         # notices the stale engines
    assert not a._stale and os.path.exists(os.path.join(a.results_folder, "sample-9.png"))
    out = a.ema.ema_model.sample([x_in], batch_size=1, noise=noise)[-1].clone()
    fresh = _two().sample([x_in], batch_size=1, noise=noise)[-1].clone()
    print(f"[measured] sample from the trained EMA of two U-Nets against the untrained model: {rel_err(out.cpu(), fresh.cpu()):.2e}")
    assert bool(torch.isfinite(out).all()) and out.shape == fresh.shape and not torch.equal(out, fresh)
    res = a.validate()
    assert len(res["loss"]) == 2 and all(len(v) == 2 and all(x == x for x in v) for v in res["loss"])
    assert all(x == x for x in res["psnr"][0]) and all(x != x for x in res["psnr"][1])          # unet1's output is no residual
    assert res["n"] == [4, 4] and a.val_log[-1] is res


def test_one_unet_with_radam(tmp_path):
    """the reference's commented-out alternative: 3 steps run, the checkpoint keeps its five keys with 'opt0' in RAdam's layout
    over all of diffusion.parameters(), and the weights are not those of the default (Adam) run on the same data"""
    from founddiff_amd.diffusion_train import CHECKPOINT_KEYS, ClipAdamEMA, ClipRAdamEMA, optimizer_kind
    tr = _trainer(tmp_path / "radam", 3, save_and_sample_every=100, optimizer="radam")
    tr.train()
    assert type(tr.opt0) is ClipRAdamEMA and tr.step == 3 and len(tr.losses) == 1
    tr.save(1)
    data = torch.load(os.path.join(tr.results_folder, "model-1.pt"), map_location="cpu", weights_only=False)
    assert sorted(data) == sorted(CHECKPOINT_KEYS) and optimizer_kind(data["opt0"]["param_groups"][0]) == "radam"
    ps = [torch.nn.Parameter(p.detach().clone()) for p in tr.model.parameters()]
    opt = torch.optim.RAdam(ps, lr=1.0)
    opt.load_state_dict(data["opt0"])
    assert len(opt.state) == len(tr.opt0.params) and all(float(st["step"]) == 3 for st in opt.state.values())
    again = _trainer(tmp_path / "radam", 3, save_and_sample_every=100, optimizer="radam")
    again.load(1, for_training=True)
    assert again.step == 3 and again.opt0.steps() == [3] * len(again.opt0.params)
    adam = _trainer(tmp_path / "adam", 3, save_and_sample_every=100)
    adam.train()
    assert type(adam.opt0) is ClipAdamEMA and adam.batch_log == tr.batch_log
    key = P0 + "init_conv.weight"
    assert not torch.equal(adam.model.state_dict()[key], tr.model.state_dict()[key])
    with pytest.raises(RuntimeError, match="RAdam"):                    # and an Adam run does not resume from RAdam's file
        _trainer(tmp_path / "radam", 3, save_and_sample_every=100).load(1, for_training=True)


def test_defaults_still_raise(tmp_path):
    """next to the opt-in: a default Trainer on the two-U-Net model raises as tests/test_own_train_cpu.py pins it"""
    tr = _trainer(tmp_path, 2, dif=_two())
    with pytest.raises(NotImplementedError, match="RAdam"):
        tr.train()
    with pytest.raises(NotImplementedError, match="RAdam"):
        tr.save(1)
    assert tr.opt0 is None and tr.model.model.unet0._trainable is None
