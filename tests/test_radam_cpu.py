"""Training two U-Nets (diffusion_train.ClipRAdamEMA, csrc/fd_train_step.hip's fd_opt_radam_ema_f32), the parts that are plain
host code: RAdam's per-step scalars against torch.optim.RAdam in float64, the checkpoint with 'opt0' and 'opt1', the C ABI of both
builds of the library, UnetRes.trainable() and the errors that fire without a GPU."""
import copy
import os
import re

import pytest
import torch

from founddiff_amd import diffusion_train as dt
from founddiff_amd.DADiff import ResidualDiffusion, Trainer, UnetRes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY_CLIP = dict(layers=(2, 1, 1, 1), width=16, embed_dim=1024)
NEW_SYMBOLS = ("fd_opt_radam_ema_f32",)


# ---- radam_scalars -------------------------------------------------------------------------------------------------------------
def _torch_radam_steps(beta2, n, lr=0.5, beta1=0.9, eps=1e-8):
    """n steps of float64 torch.optim.RAdam on a one-element parameter that is put back to 0 before every step, so that p after
    the step IS the step, without cancellation.  Per step: (-p, exp_avg, exp_avg_sq)."""
    g = torch.Generator().manual_seed(3)
    p = torch.nn.Parameter(torch.zeros(1, dtype=torch.float64))
    opt = torch.optim.RAdam([p], lr=lr, betas=(beta1, beta2), eps=eps, weight_decay=0.0)
    rows = []
    for _ in range(n):
        with torch.no_grad():
            p.zero_()
        p.grad = torch.randn(1, generator=g, dtype=torch.float64) + 2.0
        opt.step()
        st = opt.state[p]
        rows.append((-float(p.detach()), float(st["exp_avg"]), float(st["exp_avg_sq"])))
    return rows


@pytest.mark.parametrize("beta2,rho6", [(0.999, 5.99), (0.99, 5.94), (0.9, 5.39)])
def test_radam_scalars_against_torch(beta2, rho6):
    """steps 1..12: un-rectified up to step 5, rectified from step 6 on (rho = 5.99 / 5.94 / 5.39 there: at least 0.39 away from
    the threshold 5), and the step torch takes is step_size factor m / (sqrt(v) + eps), or step_size m, to 1e-12"""
    lr, beta1, eps = 0.5, 0.9, 1e-8
    rows = _torch_radam_steps(beta2, 12, lr, beta1, eps)
    b2s = beta2 ** 6
    rho = 2 / (1 - beta2) - 1 - 2 * 6 * b2s / (1 - b2s)
    assert abs(rho - rho6) < 5e-3, rho
    worst = 0.0
    for s, (moved, m, v) in enumerate(rows, start=1):
        rect, size, factor = dt.radam_scalars(s, lr, beta1, beta2)
        assert rect == (s >= 6), (s, rect)
        # which branch torch took: the un-rectified step is lr m / bc1 whatever v is
        plain = lr * m / (1 - beta1 ** s)
        assert (abs(moved - plain) > 1e-6 * abs(plain)) == rect, (s, moved, plain)
        want = size * factor * m / (v ** 0.5 + eps) if rect else size * m
        assert rect or factor == 1.0
        worst = max(worst, abs(want - moved) / abs(moved))
    print(f"[measured] radam_scalars beta2={beta2}: worst relative difference to torch.optim.RAdam's step {worst:.2e}")
    assert worst < 1e-12, worst


def test_radam_scalars_never_rectify_below_rho_inf_5():
    """beta2 = 0.5: rho_inf = 3, no step is rectified, every result is finite, and the step is torch's"""
    rows = _torch_radam_steps(0.5, 12)
    for s, (moved, m, _) in enumerate(rows, start=1):
        rect, size, factor = dt.radam_scalars(s, 0.5, 0.9, 0.5)
        assert rect is False and factor == 1.0 and size == size and abs(size) < float("inf")
        assert abs(size * m - moved) <= 1e-12 * abs(moved)
    assert dt.radam_scalars(100000, 0.5, 0.9, 0.5)[0] is False
    assert dt.radam_scalars(100000, 0.5, 0.9, 0.999)[0] is True
    with pytest.raises(RuntimeError):
        dt.radam_scalars(0, 0.5, 0.9, 0.999)


# ---- the checkpoint of two U-Nets ----------------------------------------------------------------------------------------------
def _radam_group():
    return {k: v for k, v in torch.optim.RAdam([torch.zeros(1)], lr=1e-4, weight_decay=0.0).state_dict()["param_groups"][0].items()
            if k != "params"}


def _two_unet_state():
    """a model of 7 parameters: unet0 has places 0-2, unet1 places 3-6; places 1 and 4 are frozen; the trainable ones in
    diffusion.parameters() order are 0, 2, 3, 5, 6, and the last never took a step"""
    g = torch.Generator().manual_seed(0)
    shapes = {0: (3, 2), 1: (4,), 2: (5,), 3: (3, 2), 4: (4,), 5: (5,), 6: (2, 2, 2)}
    index, unet_index = [0, 2, 3, 5, 6], ([0, 1, 2], [3, 4, 5, 6])
    m = [torch.randn(shapes[i], generator=g) for i in index]
    v = [torch.rand(shapes[i], generator=g) for i in index]
    opt_sd = dt.adam_state_pack([7, 7, 7, 4, 0], m, v, _radam_group())
    opt_sd["ema_step"], opt_sd["ema_copied"] = 7, True
    model_sd = {"model.unet0.w": torch.randn(3, 2, generator=g), "model.unet1.w": torch.randn(5, generator=g)}
    ema_sd = {k: x + 1 for k, x in model_sd.items()}
    return shapes, index, unet_index, m, v, opt_sd, model_sd, ema_sd


def test_checkpoint2_layout_round_trip():
    shapes, index, unet_index, m, v, opt_sd, model_sd, ema_sd = _two_unet_state()
    data = dt.checkpoint_pack2(12, model_sd, ema_sd, opt_sd, index, unet_index)
    assert dt.CHECKPOINT_KEYS_2 == ("step", "model", "opt0", "opt1", "ema", "scaler")
    assert dt.CHECKPOINT_KEYS == ("step", "model", "opt0", "ema", "scaler")
    assert sorted(data) == sorted(dt.CHECKPOINT_KEYS_2) and data["scaler"] is None and data["step"] == 12
    for entry, n, live in (("opt0", 3, [0, 2]), ("opt1", 4, [0, 2])):     # frozen ones, and one without a step, carry no state
        assert sorted(data[entry]) == ["param_groups", "state"]
        assert data[entry]["param_groups"][0]["params"] == list(range(n))
        assert sorted(data[entry]["state"]) == live, entry
        assert sorted(data[entry]["state"][0]) == ["exp_avg", "exp_avg_sq", "step"]
        assert dt.optimizer_kind(data[entry]["param_groups"][0]) == "radam"
    assert float(data["opt0"]["state"][2]["step"]) == 7 and float(data["opt1"]["state"][2]["step"]) == 4
    assert torch.equal(data["opt0"]["state"][2]["exp_avg"], m[1]) and torch.equal(data["opt1"]["state"][0]["exp_avg_sq"], v[2])
    assert sorted(data["ema"]) == sorted(["ema_model.model.unet0.w", "ema_model.model.unet1.w", "initted", "step"])
    # torch.optim.RAdam over each U-Net's parameters loads its entry as its own, and steps from it
    for entry, places in zip(("opt0", "opt1"), unet_index):
        ps = [torch.nn.Parameter(torch.zeros(shapes[i])) for i in places]
        opt = torch.optim.RAdam(ps, lr=1.0)
        opt.load_state_dict(copy.deepcopy(data[entry]))                   # torch keeps the step tensors it is given
        assert opt.param_groups[0]["lr"] == 1e-4 and opt.param_groups[0]["betas"] == (0.9, 0.999)
        for p in ps:
            p.grad = torch.ones_like(p)
        opt.step()
        assert float(opt.state[ps[0]]["step"]) == 8 and float(opt.state[ps[1]]["step"]) == 1
    step, model2, ema2, opt2 = dt.checkpoint_unpack2(data, index, unet_index)
    assert step == 12 and opt2["ema_step"] == 7 and opt2["ema_copied"] is True
    assert all(torch.equal(model2[k], model_sd[k]) and torch.equal(ema2[k], ema_sd[k]) for k in model_sd)
    steps, m2, v2 = dt.adam_state_unpack(opt2, len(index))
    assert steps == [7, 7, 7, 4, 0] and m2[4] is None and v2[4] is None
    assert all(torch.equal(a, b) for a, b in zip(m2[:4], m[:4])) and all(torch.equal(a, b) for a, b in zip(v2[:4], v[:4]))
    assert dt.optimizer_kind(opt2["param_groups"][0]) == "radam"


def test_checkpoint2_rejects_other_files():
    shapes, index, unet_index, m, v, opt_sd, model_sd, ema_sd = _two_unet_state()
    data = dt.checkpoint_pack2(12, model_sd, ema_sd, opt_sd, index, unet_index)
    with pytest.raises(RuntimeError, match="opt1"):                       # a one-U-Net file: another key set
        dt.checkpoint_unpack2({k: x for k, x in data.items() if k != "opt1"}, index, unet_index)
    with pytest.raises(RuntimeError):                                     # and the other way round
        dt.checkpoint_unpack(data, index, 7)
    adam = {k: x for k, x in torch.optim.Adam([torch.zeros(1)]).state_dict()["param_groups"][0].items() if k != "params"}
    assert dt.optimizer_kind(adam) == "adam" and dt.optimizer_kind({"lr": 1.0}) is None
    bad = dict(data, opt0=dict(data["opt0"], param_groups=[dict(adam, params=[0, 1, 2])]))
    with pytest.raises(RuntimeError, match="(?s)Adam.*RAdam"):
        dt.checkpoint_unpack2(bad, index, unet_index)
    # the five-key checkpoint: the optimiser is checked on request, and not otherwise (as before)
    one = dt.checkpoint_pack(3, model_sd, ema_sd, dt.adam_state_pack([1, 1], m[:2], v[:2], _radam_group()), [0, 2], 3)
    assert sorted(one) == sorted(dt.CHECKPOINT_KEYS) and dt.optimizer_kind(one["opt0"]["param_groups"][0]) == "radam"
    dt.checkpoint_unpack(one, [0, 2], 3)
    dt.checkpoint_unpack(one, [0, 2], 3, optimizer="radam")
    with pytest.raises(RuntimeError, match="(?s)RAdam.*Adam"):
        dt.checkpoint_unpack(one, [0, 2], 3, optimizer="adam")
    with pytest.raises(RuntimeError, match="frozen"):                     # state for a frozen parameter
        dt.checkpoint_unpack2(data, [0, 3, 5, 6], unet_index)
    with pytest.raises(RuntimeError, match="neither"):
        dt.checkpoint_pack2(12, model_sd, ema_sd, opt_sd, index, ([0, 1, 2], [3, 4, 5]))


# ---- symbols -------------------------------------------------------------------------------------------------------------------
def test_new_entries_are_declared_and_exported():
    """declared in include/founddiff_hip.h, present in _lib's table with the Adam entry's signature, exported by both builds"""
    from founddiff_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "founddiff_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint " + name + r"\(", hdr), name
        assert name in L.SIGNATURES, name
    assert L.SIGNATURES["fd_opt_radam_ema_f32"] == L.SIGNATURES["fd_opt_adam_ema_f32"]
    for build in (L.BF16, L.F16):
        lib = build.lib()
        for name in NEW_SYMBOLS:
            assert hasattr(lib, name), name
    assert dt.ClipRAdamEMA._update_entry == "fd_opt_radam_ema_f32" and dt.ClipAdamEMA._update_entry == "fd_opt_adam_ema_f32"
    assert issubclass(dt.ClipRAdamEMA, dt.ClipAdamEMA)


# ---- UnetRes.trainable() -------------------------------------------------------------------------------------------------------
def _diffusion(num_unet=2, objective="pred_res_noise"):
    net = UnetRes(64, dim_mults=(1, 2), num_unet=num_unet, condition=True, objective=objective, clip_cfg=TINY_CLIP)
    return ResidualDiffusion(net, image_size=64, objective=objective, condition=True)


def test_unetres_trainable_views():
    dif = _diffusion()
    net = dif.model
    assert net.unet0._trainable is None and net.unet1._trainable is None
    views = net.trainable()
    assert isinstance(views, list) and len(views) == 2 and views[0] is net.unet0.trainable() and views[1] is net.unet1.trainable()
    for u, view in zip((net.unet0, net.unet1), views):
        mine, theirs = dict(u.named_parameters()), dict(view.named_parameters())
        trunk = [k for k in mine if not k.startswith("dose_encoder.")]
        assert sorted(trunk) == sorted(theirs)
        assert all(theirs[k] is mine[k] and theirs[k].data_ptr() == mine[k].data_ptr() and mine[k].requires_grad for k in trunk)
        assert not any(p.requires_grad for k, p in mine.items() if k.startswith("dose_encoder."))
    assert views[0].init_conv.weight.data_ptr() != views[1].init_conv.weight.data_ptr()
    assert sorted(dif.state_dict()) == sorted(_diffusion().state_dict())          # the views are no sub-modules
    c = dif.clone()                                                               # a deep copy: views over its own parameters
    for name in ("unet0", "unet1"):
        cu, u = getattr(c.model, name), getattr(net, name)
        assert cu.trainable().init_conv.weight is cu.init_conv.weight
        assert cu.init_conv.weight.data_ptr() != u.init_conv.weight.data_ptr()
    assert len(UnetRes(64, dim_mults=(1, 2), num_unet=1, condition=True, objective="pred_res", clip_cfg=TINY_CLIP).trainable()) == 1


def test_opt_in_message_names_the_switches():
    dif = _diffusion()
    imgs = [torch.rand(2, 1, 64, 64), torch.rand(2, 1, 64, 64)]
    with pytest.raises(NotImplementedError, match="RAdam") as e:
        dif(imgs)
    assert "model.trainable()" in str(e.value) and 'Trainer(optimizer="radam")' in str(e.value)
    dif.model.unet0.trainable()                                                   # one view only: still not trainable
    with pytest.raises(NotImplementedError, match="RAdam"):
        dif(imgs)
    dif.model.trainable()                                                         # opted in: the call now reaches the device checks
    with pytest.raises(RuntimeError, match="no CPU path"):
        dif(imgs)


# ---- Trainer -------------------------------------------------------------------------------------------------------------------
def test_trainer_optimizer_argument(tmp_path):
    imgs = [torch.rand(1, 64, 64), torch.rand(1, 64, 64)]
    with pytest.raises(RuntimeError, match="optimizer"):
        Trainer(None, _diffusion(), checkpoint_folder=str(tmp_path), device="cpu", train_dataset=[imgs], optimizer="sgd")
    for n, objective in ((2, "pred_res_noise"), (1, "pred_res")):
        tr = Trainer(None, _diffusion(n, objective), checkpoint_folder=str(tmp_path), device="cpu", train_dataset=[imgs],
                     optimizer="radam")
        assert tr.optimizer == "radam" and tr.radam_betas == (0.9, 0.999) and tr.opt0 is None and not hasattr(tr, "opt1")
        with pytest.raises(RuntimeError, match="no CPU path"):
            tr.train()
        with pytest.raises(RuntimeError, match="no CPU path"):
            tr.save(1)
    tr = Trainer(None, _diffusion(), checkpoint_folder=str(tmp_path), device="cpu", train_dataset=[imgs], optimizer="adam")
    with pytest.raises(NotImplementedError, match="optimizer='radam'"):
        tr.train()
    assert Trainer(None, _diffusion(1, "pred_res"), checkpoint_folder=str(tmp_path), device="cpu").optimizer == "adam"
