"""founddiff_amd.diffusion_train (csrc/fd_train_step.hip) on the GPU: q_sample, the loss, the fused clip + Adam + EMA optimiser, its
checkpoint entry, one whole training step of a small trunk and the binding on the reference's attribute names.

References are float64 restatements of the reference's lines (src/DADiff.py:1382-1388, 1476-1481, 1493-1497) and float64
clip_grad_norm_ + torch.optim.Adam on the CPU.  Gates, the project's training gates: rel_err < 1e-5 (OUT) for outputs and optimiser
state, < 1e-4 (ACT) for the parameter movement, < 1e-4 (CAPTURE) for the first loss of a whole step.  Every test prints what it
measured."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err

pytestmark = pytest.mark.gpu

ACT, OUT, CAPTURE = 1e-4, 1e-5, 1e-4
T = 1000


def _report(tag, errs):
    print(f"[measured] {tag}: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))


def _schedule():
    from founddiff_amd.DADiff import residual_schedule
    return residual_schedule(T)


# ---- 1. q_sample -------------------------------------------------------------------------------------------------------------------
QS_SHAPES = [(1, 1, 1), (2, 3, 5), (3, 1, 257), (2, 130, 70)]
_TS = {1: [T - 1], 2: [0, T - 1], 3: [0, 500, T - 1]}


def _qs_inputs(shape, seed=3):
    B, H, W = shape
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, 1, H, W, generator=g), torch.rand(B, 1, H, W, generator=g), torch.tensor(_TS[B]),
            torch.randn(B, 1, H, W, generator=g))


def _qs_float64(x0, xi, t, noise, sch, normalize=True):
    """src/DADiff.py:1493-1497, 1412, 1382-1388, 1436, 1439-1440 in float64"""
    x0, xi, noise = x0.double(), xi.double(), noise.double()
    if normalize:
        x0, xi = x0 * 2 - 1, xi * 2 - 1
    ac, bc = sch["alphas_cumsum"].double()[t], sch["betas_cumsum"].double()[t]
    x_res = xi - x0
    x = x0 + ac.view(-1, 1, 1, 1) * x_res + bc.view(-1, 1, 1, 1) * noise
    return dict(x_in=torch.cat((x, xi), dim=1), x_res=x_res, times=torch.stack((ac * T, bc * T)))


@pytest.mark.parametrize("normalize", [True, False], ids=["norm", "raw"])
@pytest.mark.parametrize("shape", QS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_q_sample_given_noise(shape, normalize):
    """x_in, x_res and times against float64 at OUT; plane 1 is 2 x_input - 1 bit for bit; the given noise comes back as it is; no
    input changes"""
    from founddiff_amd.diffusion_train import q_sample
    sch = _schedule()
    x0, xi, t, nz = _qs_inputs(shape)
    dev = [v.cuda() for v in (x0, xi, t, nz)]
    keep = [v.clone() for v in dev]
    x_in, x_res, noise, times = q_sample(dev[0], dev[1], dev[2], sch, noise=dev[3], normalize=normalize)
    ref = _qs_float64(x0, xi, t, nz, sch, normalize)
    B, H, W = shape
    assert x_in.shape == (B, 2, H, W) and x_res.shape == (B, 1, H, W) and times.shape == (2, B) and noise is dev[3]
    errs = dict(x_in=rel_err(x_in.cpu(), ref["x_in"]), x_res=rel_err(x_res.cpu(), ref["x_res"]), times=rel_err(times.cpu(), ref["times"]))
    _report(f"q_sample {shape} normalize={normalize}", errs)
    assert all(e < OUT for e in errs.values()), errs
    assert torch.equal(x_in[:, 1:2].cpu(), xi * 2 - 1 if normalize else xi)
    assert all(torch.equal(a, b) for a, b in zip(dev, keep))


@pytest.mark.parametrize("shape", QS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_q_sample_keyed_noise(shape):
    """with seeds the noise is fd_keyed_normal(seeds, step) bit for bit, agrees with its numpy restatement as
    test_keyed_noise_kernels_vs_oracle checks that entry (5e-5 absolute), and x_t is built from it; slice 1 of a batch gets the
    bits it gets alone"""
    from founddiff_amd import _lib as L
    from founddiff_amd.diffusion_train import q_sample
    from oracle import keyed_noise as kn
    sch = _schedule()
    x0, xi, t, _ = _qs_inputs(shape)
    B, H, W = shape
    npix = H * W
    step = 12345
    seeds = torch.tensor([5, (1 << 40) + 17, 123456789012345][:B], dtype=torch.int64)
    dev = [v.cuda() for v in (x0, xi, t, seeds)]
    keep = [v.clone() for v in dev]
    x_in, x_res, noise, times = q_sample(dev[0], dev[1], dev[2], sch, slice_seeds=dev[3], step=step)
    want = torch.empty(B, npix, device="cuda")
    L.call("fd_keyed_normal", dev[3].data_ptr(), step, want.data_ptr(), B, npix, torch.cuda.current_stream().cuda_stream)
    assert noise.shape == (B, 1, H, W) and torch.equal(noise.view(B, npix), want)
    ref_noise = torch.from_numpy(np.stack([kn.keyed_normal(int(s), step, npix) for s in seeds.tolist()]))
    e_noise = float((noise.view(B, npix).cpu() - ref_noise).abs().max())
    ref = _qs_float64(x0, xi, t, noise.cpu(), sch)
    errs = dict(noise_abs=e_noise, x_in=rel_err(x_in.cpu(), ref["x_in"]), x_res=rel_err(x_res.cpu(), ref["x_res"]))
    _report(f"q_sample keyed {shape}", errs)
    assert e_noise < 5e-5 and errs["x_in"] < OUT and errs["x_res"] < OUT, errs
    assert all(torch.equal(a, b) for a, b in zip(dev, keep))
    if B > 1:
        k = 1
        alone = q_sample(dev[0][k:k + 1], dev[1][k:k + 1], dev[2][k:k + 1], sch, slice_seeds=dev[3][k:k + 1], step=step)
        for a, b in zip(alone[:3], (x_in, x_res, noise)):
            assert torch.equal(a, b[k:k + 1])
        assert torch.equal(alone[3], times[:, k:k + 1])


# ---- 2. the loss -------------------------------------------------------------------------------------------------------------------
LOSS_SHAPES = [(1, 1), (2, 15), (3, 4097), (2, 9100)]


def _loss_inputs(B, npix, seed=11):
    g = torch.Generator().manual_seed(seed)
    pred, target = torch.randn(B, 1, npix, generator=g), torch.randn(B, 1, npix, generator=g)
    ties = torch.rand(B, 1, npix, generator=g) < 0.1
    if npix == 1:
        ties[:] = False
    target = torch.where(ties, pred, target)
    return pred, target, ties


def _loss_float64(pred, target, loss_type, scale):
    """src/DADiff.py:1478-1480 in float64, with autograd's gradient"""
    p = pred.double().requires_grad_()
    loss = (F.l1_loss if loss_type == "l1" else F.mse_loss)(p, target.double(), reduction="none")
    loss = loss.flatten(1).mean(dim=1).mean() * scale
    return loss.detach(), torch.autograd.grad(loss, p)[0]


@pytest.mark.parametrize("scale", [1.0, 0.25])
@pytest.mark.parametrize("loss_type", ["l1", "l2"])
@pytest.mark.parametrize("shape", LOSS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_residual_loss(shape, loss_type, scale):
    """loss and dpred against float64 autograd at OUT; dpred exactly 0 at the ties for l1; two runs equal bit for bit; an incoming
    gradient of 3 scales dpred by 3; the target gets no gradient and the inputs do not change"""
    from founddiff_amd.diffusion_train import residual_loss
    B, npix = shape
    pred, target, ties = _loss_inputs(B, npix)
    l64, d64 = _loss_float64(pred, target, loss_type, scale)
    p, tg = pred.cuda().requires_grad_(), target.cuda().requires_grad_()
    keep = p.detach().clone(), tg.detach().clone()
    loss = residual_loss(p, tg, loss_type, scale)
    assert loss.shape == () and loss.is_cuda
    dp, dt_ = torch.autograd.grad(loss, [p, tg], allow_unused=True, retain_graph=True)
    assert dt_ is None
    errs = dict(loss=abs(float(loss.detach()) - float(l64)) / abs(float(l64)), dpred=rel_err(dp.cpu(), d64))
    _report(f"loss {loss_type} {shape} scale={scale}", errs)
    assert all(e < OUT for e in errs.values()), errs
    if loss_type == "l1":
        assert bool((dp.cpu()[ties] == 0).all()) and bool((dp.cpu()[~ties] != 0).all())
    dp3, = torch.autograd.grad(loss, [p], torch.tensor(3.0, device="cuda"))
    assert torch.equal(dp3, 3.0 * dp)
    loss2 = residual_loss(p, tg, loss_type, scale)
    dp2, = torch.autograd.grad(loss2, [p])
    assert torch.equal(loss2, loss) and torch.equal(dp2, dp)
    assert torch.equal(p.detach(), keep[0]) and torch.equal(tg.detach(), keep[1])


# ---- 3-7. the optimiser ------------------------------------------------------------------------------------------------------------
OPT_SHAPES = [(1,), (3,), (5,), (64,), (1023,), (4096,), (4097,), (7, 9, 3, 3), (128, 33), (70001,)]
K_MISALIGNED, K_NOGRAD, K_4097 = len(OPT_SHAPES), len(OPT_SHAPES) + 1, 6
N_MIS, N_NOGRAD = 777, 50
NT = len(OPT_SHAPES) + 2
STEPS, LR, BETAS = 5, 1e-2, (0.9, 0.99)
_SCALES = (1e-4, 1.0, 30.0)


def _opt_host(seed=21):
    """initial values of the twelve parameters and of their EMA copies, and the gradients of STEPS steps: randn times 1e-4 / 1 / 30
    rotating per tensor on the even steps (clipping active), times 1e-4 (1 + i % 3) on the odd ones (the total norm stays below
    1: no clipping).  The last parameter never gets a gradient."""
    g = torch.Generator().manual_seed(seed)
    shapes = OPT_SHAPES + [(N_MIS,), (N_NOGRAD,)]
    p0 = [torch.randn(s, generator=g) for s in shapes]
    e0 = [torch.randn(s, generator=g) for s in shapes]
    grads = []
    for s in range(STEPS):
        row = []
        for i, shp in enumerate(shapes):
            k = _SCALES[(s // 2 + i) % 3] if s % 2 == 0 else 1e-4 * (1 + i % 3)
            row.append(None if i == K_NOGRAD else k * torch.randn(shp, generator=g))
        grads.append(row)
    return p0, e0, grads


def _on_gpu(values):
    """the values as parameters on the GPU; the misaligned one sits one float behind a 16-byte boundary"""
    out = []
    for i, v in enumerate(values):
        if i == K_MISALIGNED:
            t = torch.empty(v.numel() + 1, device="cuda")[1:]
            assert t.data_ptr() % 16 == 4
            t.copy_(v)
        else:
            t = v.cuda()
        out.append(t.requires_grad_())
    return out


def _set_grads(params, row, alias=None):
    for i, (p, g) in enumerate(zip(params, row)):
        if g is None:
            p.grad = None
        elif p.grad is None:
            if i == K_MISALIGNED:
                buf = torch.empty(g.numel() + 1, device="cuda")[1:]
                buf.copy_(g)
                p.grad = buf
            else:
                p.grad = g.cuda()
        else:
            p.grad.copy_(g)


_REF = {}


def _opt_float64():
    """float64 clip_grad_norm_(1.0) + torch.optim.Adam on the CPU: per step the total norm, exp_avg, exp_avg_sq; the final
    parameters and step counts.  Computed once."""
    if not _REF:
        p0, _, grads = _opt_host()
        ps = [torch.nn.Parameter(v.double()) for v in p0]
        opt = torch.optim.Adam(ps, lr=LR, betas=BETAS)
        norms, ms, vs = [], [], []
        for row in grads:
            for p, g in zip(ps, row):
                p.grad = None if g is None else g.double()
            norms.append(float(torch.nn.utils.clip_grad_norm_(ps, 1.0)))
            opt.step()
            ms.append([opt.state[p]["exp_avg"].clone() if p in opt.state else None for p in ps])
            vs.append([opt.state[p]["exp_avg_sq"].clone() if p in opt.state else None for p in ps])
        steps = [int(opt.state[p]["step"]) if p in opt.state else 0 for p in ps]
        _REF.update(norms=norms, m=ms, v=vs, p=[p.detach() for p in ps], steps=steps)
    return _REF


def _run_fused(zero_grad=True, **kw):
    """the STEPS steps on the GPU: everything the tests compare"""
    from founddiff_amd.diffusion_train import ClipAdamEMA
    p0, e0, grads = _opt_host()
    params, ema = _on_gpu(p0), [v.cuda() for v in e0]
    opt = ClipAdamEMA(params, ema, lr=LR, betas=BETAS, **kw)
    out = dict(norms=[], coefs=[], flags=[], m=[], v=[], grads_after=[])
    for row in grads:
        _set_grads(params, row)
        rec = opt.step(zero_grad=zero_grad).clone()
        out["norms"].append(rec[0]), out["coefs"].append(rec[1]), out["flags"].append(rec[2])
        out["m"].append([m.clone() for m in opt.exp_avg])
        out["v"].append([v.clone() for v in opt.exp_avg_sq])
        out["grads_after"].append([None if p.grad is None else p.grad.clone() for p in params])
    out.update(p=[p.detach().clone() for p in params], ema=[e.clone() for e in ema], steps=opt.steps(), opt=opt, params=params)
    return out


def _p_metric(p, p64, p64_before):
    return float((p.double().cpu() - p64).abs().max() / (p64 - p64_before).abs().max())


def test_optimiser_against_float64():
    """5 steps of clip + Adam on twelve tensors (sizes around the 4096-element chunk, a 4-D one, a misaligned one, one without a
    gradient): the parameter movement at ACT, exp_avg, exp_avg_sq and the total norm per step at OUT, equal step counts; clipping
    is active on the even steps and not on the odd ones; the gradients are zero afterwards"""
    ref, got = _opt_float64(), _run_fused()
    p0, _, grads = _opt_host()
    assert [n > 1 for n in ref["norms"]] == [True, False, True, False, True]
    errs = dict(p=0.0, exp_avg=0.0, exp_avg_sq=0.0, total_norm=0.0)
    for i in range(NT):
        if i == K_NOGRAD:
            continue
        errs["p"] = max(errs["p"], _p_metric(got["p"][i], ref["p"][i], p0[i].double()))
        for s in range(STEPS):
            errs["exp_avg"] = max(errs["exp_avg"], rel_err(got["m"][s][i].cpu(), ref["m"][s][i]))
            errs["exp_avg_sq"] = max(errs["exp_avg_sq"], rel_err(got["v"][s][i].cpu(), ref["v"][s][i]))
    for s in range(STEPS):
        errs["total_norm"] = max(errs["total_norm"], abs(float(got["norms"][s]) - ref["norms"][s]) / ref["norms"][s])
        coef = float(got["coefs"][s])
        assert (coef < 1) == (ref["norms"][s] > 1) and float(got["flags"][s]) == 0, (s, coef)
    _report("optimiser, 5 steps", errs)
    assert errs["p"] < ACT and errs["exp_avg"] < OUT and errs["exp_avg_sq"] < OUT and errs["total_norm"] < OUT, errs
    assert got["steps"] == ref["steps"] == [STEPS] * (NT - 1) + [0]
    k = K_NOGRAD                                                         # the parameter without a gradient: nothing moved
    assert torch.equal(got["p"][k].cpu(), p0[k]) and not got["m"][-1][k].any() and not got["v"][-1][k].any()
    assert got["params"][k].grad is None
    for row in got["grads_after"]:
        assert all(g is None or not g.any() for g in row)


def test_optimiser_keeps_gradients_without_the_fold():
    """step(zero_grad=False) leaves every gradient as it was, and the update is the same"""
    a, b = _run_fused(), _run_fused(zero_grad=False)
    _, _, grads = _opt_host()
    for s in range(STEPS):
        for g, want in zip(b["grads_after"][s], grads[s]):
            assert (g is None and want is None) or torch.equal(g.cpu(), want)
    assert all(torch.equal(x, y) for x, y in zip(a["p"], b["p"]))


def test_ema_modes():
    """mode 1 copies the new parameters bit for bit; mode 2 with decay 0.5 and 0.995 against float64 at OUT (on the value: the
    movement is dominated by ulp(p)); mode 0 and a parameter without a gradient leave the EMA alone"""
    from founddiff_amd.diffusion_train import ClipAdamEMA
    p0, e0, grads = _opt_host()
    for mode, decay in ((0, None), (1, None), (2, 0.5), (2, 0.995)):
        params, ema = _on_gpu(p0), [v.cuda() for v in e0]
        opt = ClipAdamEMA(params, ema, lr=LR, betas=BETAS)
        _set_grads(params, grads[0])
        opt.step(ema_mode=mode, ema_decay=decay)
        worst = 0.0
        for i in range(NT):
            if i == K_NOGRAD or mode == 0:
                assert torch.equal(ema[i].cpu(), e0[i])
            elif mode == 1:
                assert torch.equal(ema[i], params[i].detach())
            else:
                e64 = e0[i].double() - (1 - decay) * (e0[i].double() - params[i].detach().double().cpu())
                worst = max(worst, rel_err(ema[i].cpu(), e64))
        if mode == 2:
            _report(f"ema mode 2 decay {decay}", dict(ema=worst))
            assert worst < OUT, worst


def test_ema_schedule_on_the_device():
    """25 steps with update_every=2, update_after_step=4 against the float64 restatement of the rule (ema-pytorch's, as the
    reference constructs it) fed with the GPU's parameters: OUT"""
    from founddiff_amd.diffusion_train import ClipAdamEMA
    p0, e0, grads = _opt_host()
    params, ema = _on_gpu(p0), [v.cuda() for v in e0]
    opt = ClipAdamEMA(params, ema, lr=1e-3, betas=BETAS, ema_update_every=2, ema_update_after_step=4)
    e64 = [v.double() for v in e0]
    s, copied, modes = 0, False, []
    for k in range(25):
        _set_grads(params, grads[k % STEPS])
        opt.step()
        p64 = [p.detach().double().cpu() for p in params]
        s0 = s
        s += 1
        if s0 % 2 != 0:
            modes.append(0)
            continue
        if s0 <= 4:
            e64, copied = [v.clone() for v in p64], True
            modes.append(1)
            continue
        if not copied:
            e64, copied = [v.clone() for v in p64], True
        epoch = max(s - 4 - 1, 0)
        decay = 0.0 if epoch <= 0 else min(max(1 - (1 + epoch / 1.0) ** -(2 / 3), 0.0), 0.995)
        e64 = [e - (1 - decay) * (e - p) for e, p in zip(e64, p64)]
        modes.append(2)
    assert modes.count(1) == 3 and modes.count(2) == 10
    worst = max(rel_err(ema[i].cpu(), e64[i]) for i in range(NT) if i != K_NOGRAD)
    _report("ema schedule, 25 steps", dict(ema=worst))
    assert worst < OUT, worst
    assert torch.equal(ema[K_NOGRAD].cpu(), e0[K_NOGRAD])


@pytest.mark.parametrize("k", [K_4097, K_MISALIGNED], ids=["4097", "misaligned"])
def test_update_does_not_depend_on_the_other_tensors(k):
    """max_norm=None: p, exp_avg and exp_avg_sq of tensor k after 3 steps are the same bits whether the list holds all twelve
    tensors or tensor k alone"""
    from founddiff_amd.diffusion_train import ClipAdamEMA
    p0, _, grads = _opt_host()
    params = _on_gpu(p0)
    opt = ClipAdamEMA(params, lr=LR, betas=BETAS, max_norm=None)
    if k == K_MISALIGNED:
        solo = torch.empty(p0[k].numel() + 1, device="cuda")[1:].copy_(p0[k]).requires_grad_()
    else:
        solo = p0[k].cuda().requires_grad_()
    opt1 = ClipAdamEMA([solo], lr=LR, betas=BETAS, max_norm=None)
    for s in range(3):
        _set_grads(params, grads[s])
        solo.grad = params[k].grad.clone() if k != K_MISALIGNED else torch.empty(p0[k].numel() + 1, device="cuda")[1:].copy_(params[k].grad)
        rec, rec1 = opt.step(), opt1.step()
        assert float(rec[1]) == 1.0 and float(rec1[1]) == 1.0
    assert torch.equal(solo.detach(), params[k].detach())
    assert torch.equal(opt1.exp_avg[0], opt.exp_avg[k]) and torch.equal(opt1.exp_avg_sq[0], opt.exp_avg_sq[k])
    assert opt1.steps() == [3]


def test_optimiser_is_deterministic():
    """two runs of the five steps agree bit for bit in everything, the total norm included"""
    a, b = _run_fused(), _run_fused()
    for key in ("p", "ema"):
        assert all(torch.equal(x, y) for x, y in zip(a[key], b[key])), key
    for key in ("norms", "coefs"):
        assert all(torch.equal(x, y) for x, y in zip(a[key], b[key])), key
    for key in ("m", "v"):
        assert all(torch.equal(x, y) for ra, rb in zip(a[key], b[key]) for x, y in zip(ra, rb)), key
    assert a["steps"] == b["steps"]


def test_nonfinite_step_is_skipped():
    """skip_nonfinite=True and one inf in one gradient: p, exp_avg, exp_avg_sq, the EMA and the step counts keep their bits, the
    record's flag is 1; the next finite step proceeds"""
    from founddiff_amd.diffusion_train import ClipAdamEMA
    p0, e0, grads = _opt_host()
    params, ema = _on_gpu(p0), [v.cuda() for v in e0]
    opt = ClipAdamEMA(params, ema, lr=LR, betas=BETAS, skip_nonfinite=True)
    _set_grads(params, grads[0])
    assert float(opt.step()[2]) == 0
    snap = lambda: ([p.detach().clone() for p in params], [m.clone() for m in opt.exp_avg], [v.clone() for v in opt.exp_avg_sq],
                    [e.clone() for e in ema], opt.steps())
    before = snap()
    _set_grads(params, grads[1])
    params[K_4097].grad[4096] = float("inf")
    rec = opt.step(ema_mode=1).clone()
    after = snap()
    assert float(rec[2]) == 1 and not torch.isfinite(rec[0])
    for x, y in zip(before[:4], after[:4]):
        assert all(torch.equal(a, b) for a, b in zip(x, y))
    assert before[4] == after[4] == [1] * (NT - 1) + [0]
    _set_grads(params, grads[2])
    rec = opt.step().clone()
    assert float(rec[2]) == 0 and opt.steps() == [2] * (NT - 1) + [0]
    assert all(not torch.equal(p.detach(), b) for i, (p, b) in enumerate(zip(params, before[0])) if i != K_NOGRAD)
    assert all(bool(torch.isfinite(p).all()) for p in params)


def test_checkpoint_entry():
    """two steps of a GPU torch.optim.Adam, its state dict loaded into ClipAdamEMA, one more step on each with the same gradients:
    the gates of the optimiser test; and torch.optim.Adam loads what ClipAdamEMA saves and takes a step"""
    from founddiff_amd.diffusion_train import ClipAdamEMA
    p0, _, grads = _opt_host()
    tp = [torch.nn.Parameter(v.cuda()) for v in p0]
    adam = torch.optim.Adam(tp, lr=LR, betas=BETAS)
    for s in range(2):
        for p, g in zip(tp, grads[s]):
            p.grad = None if g is None else g.cuda()
        adam.step()
    params = _on_gpu([p.detach().cpu() for p in tp])
    before = [p.detach().double().cpu() for p in tp]
    opt = ClipAdamEMA(params, lr=1.0, betas=(0.5, 0.5), max_norm=None)
    opt.load_state_dict(adam.state_dict())
    assert opt.lr == LR and opt.betas == BETAS and opt.steps() == [2] * (NT - 1) + [0]
    for p, g in zip(tp, grads[2]):
        p.grad = None if g is None else g.cuda()
    adam.step()
    _set_grads(params, grads[2])
    opt.step()
    errs = dict(p=0.0, exp_avg=0.0, exp_avg_sq=0.0)
    for i in range(NT - 1):
        st = adam.state[tp[i]]
        errs["p"] = max(errs["p"], _p_metric(params[i].detach(), tp[i].detach().double().cpu(), before[i]))
        errs["exp_avg"] = max(errs["exp_avg"], rel_err(opt.exp_avg[i].cpu(), st["exp_avg"].cpu()))
        errs["exp_avg_sq"] = max(errs["exp_avg_sq"], rel_err(opt.exp_avg_sq[i].cpu(), st["exp_avg_sq"].cpu()))
        assert int(st["step"]) == 3
    _report("checkpoint: one step after load_state_dict", errs)
    assert errs["p"] < ACT and errs["exp_avg"] < OUT and errs["exp_avg_sq"] < OUT, errs
    assert opt.steps() == [3] * (NT - 1) + [0]
    sd = opt.state_dict()
    assert sorted(sd["state"]) == list(range(NT - 1)) and sd["ema_step"] == 1
    tq = [torch.nn.Parameter(p.detach().clone()) for p in params]
    other = torch.optim.Adam(tq, lr=1.0)
    other.load_state_dict(sd)
    for p, g in zip(tq, grads[3]):
        p.grad = None if g is None else g.cuda()
    other.step()
    assert float(other.state[tq[0]]["step"]) == 4 and other.param_groups[0]["lr"] == LR
    assert torch.equal(other.state[tq[K_4097]]["exp_avg_sq"] > 0, torch.ones_like(tq[K_4097], dtype=torch.bool))
    assert all(bool(torch.isfinite(p).all()) for p in tq)


# ---- 8. a whole step ---------------------------------------------------------------------------------------------------------------
def _sinusoidal_emb(x, dim):
    """oracle.nets.sinusoidal_emb in the dtype of x"""
    import math
    half = dim // 2
    f = torch.exp(torch.arange(half, dtype=x.dtype) * -(math.log(10000) / (half - 1)))
    a = x[:, None] * f[None, :]
    return torch.cat((a.sin(), a.cos()), dim=-1)


def _step_inputs():
    """the weights and inputs of tests/test_gpu_resample_train.py::test_trunk_gradients_against_float64, and a batch"""
    from founddiff_amd import arch, synth
    spec = {k: v for k, v in arch.da_unet_spec(64, (1, 2)).items() if not k.startswith("dose_encoder.")}
    g = torch.Generator().manual_seed(41)
    sd = synth.synth_state_dict(spec, 5)
    for k in sd:
        if "adaLN_modulation.1." in k:
            sd[k] = 0.05 * torch.randn(sd[k].shape, generator=g)
    dose = torch.randn(2, 1024, generator=g)
    dose = dose / dose.norm(dim=-1, keepdim=True)
    c = F.normalize(torch.randn(2, 1, 256, generator=g), dim=-1)
    x_start, x_input = torch.rand(2, 1, 16, 16, generator=g), torch.rand(2, 1, 16, 16, generator=g)
    noise = torch.randn(2, 1, 16, 16, generator=g)
    return sd, dose, c, x_start, x_input, torch.tensor([700, 20]), noise


def cpu_train_loop(dtype, objective, loss_type, steps=5, lr=1e-3):
    """the loop body of Trainer.train on the CPU in `dtype`: the reference's p_losses lines, oracle.nets.da_unet with the torch
    scan, clip_grad_norm_(1.0) + torch.optim.Adam(betas=(0.9, 0.99)).  Returns the losses."""
    from oracle import nets
    sd, dose, c, x_start, x_input, t, noise = _step_inputs()
    sch = _schedule()
    acs, bcs = sch["alphas_cumsum"].to(dtype), sch["betas_cumsum"].to(dtype)
    ps = {k: v.to(dtype).clone().requires_grad_() for k, v in sd.items()}
    opt = torch.optim.Adam(list(ps.values()), lr=lr, betas=(0.9, 0.99))
    x0, xi, nz, dose, c = (v.to(dtype) for v in (x_start * 2 - 1 if dtype == torch.float32 else x_start.double() * 2 - 1,
                                                 x_input * 2 - 1 if dtype == torch.float32 else x_input.double() * 2 - 1, noise, dose, c))
    real, nets.sinusoidal_emb = nets.sinusoidal_emb, _sinusoidal_emb
    losses = []
    try:
        for _ in range(steps):
            x_res = xi - x0
            x = x0 + acs[t].view(-1, 1, 1, 1) * x_res + bcs[t].view(-1, 1, 1, 1) * nz
            time = (acs[t] if objective == "pred_res" else bcs[t]) * T
            tm = F.linear(F.silu(F.linear(dose, ps["text_mlp.0.weight"], ps["text_mlp.0.bias"])), ps["text_mlp.2.weight"],
                          ps["text_mlp.2.bias"])
            pe = F.linear(torch.softmax(tm, dim=1) * ps["prompt"], ps["prompt_mlp.weight"], ps["prompt_mlp.bias"])
            out = nets.da_unet(nets.SD(ps), torch.cat((x, xi), dim=1), time, cond=(c, pe), scan_fn=nets.selective_scan_torch)
            target = x_res if objective == "pred_res" else nz
            loss = (F.l1_loss if loss_type == "l1" else F.mse_loss)(out, target, reduction="none").flatten(1).mean(dim=1).mean()
            loss.backward()
            torch.nn.utils.clip_grad_norm_(list(ps.values()), 1.0)
            opt.step()
            opt.zero_grad()
            losses.append(float(loss))
    finally:
        nets.sinusoidal_emb = real
    return losses


# measured on the CPU: max over steps 2-5 of |loss32[k] - loss64[k]| / loss64[0] of cpu_train_loop(float32) against
# cpu_train_loop(float64): see the docstring of test_whole_step
STEP_GATES = {("pred_res", "l2"): 3.27e-5, ("pred_noise", "l1"): 1.35e-6}


@pytest.mark.parametrize("objective,loss_type", [("pred_res", "l2"), ("pred_noise", "l1")])
def test_whole_step(objective, loss_type):
    """UnetTrunk(64, (1, 2)) with the weights of test_trunk_gradients_against_float64, random normalised dose_embedding and c, a
    batch of two 16 x 16 slices, t = (700, 20), given noise: 5 train_steps at lr 1e-3 (the EMA list starts one off the parameters)
    against the same loop in float64 on the CPU (cpu_train_loop: the reference's p_losses lines, oracle.nets.da_unet, float64
    clip + Adam).  The first loss at CAPTURE.  Losses 2-5 as |loss[k] - loss64[k]| / loss64[0] below a measured gate: Adam's first
    steps are +-lr sign(g), so parameters whose gradient is zero analytically move by rounding noise and two correct fp32
    trajectories differ -- cpu_train_loop(float32) against cpu_train_loop(float64) on the CPU gave at most
    3.27e-5 (pred_res / l2, at step 2) and 1.35e-6 (pred_noise / l1, at step 4); the gate is 10 times that, not below CAPTURE:
    3.27e-4 and 1e-4.  Parameters are not compared element by element.  Every loss is finite, the EMA equals the parameters
    after step 1 (the schedule's first call copies) and the gradients are zero after every step."""
    from founddiff_amd.diffusion_train import ClipAdamEMA, train_step
    from founddiff_amd.unet_train import UnetTrunk
    sd, dose, c, x_start, x_input, t, noise = _step_inputs()
    l64 = cpu_train_loop(torch.float64, objective, loss_type)
    m = UnetTrunk(64, (1, 2))
    m.load_state_dict(sd, strict=True)
    m = m.cuda()
    twin = copy.deepcopy(m)
    with torch.no_grad():
        for p in twin.parameters():
            p.add_(1.0)
    params, ema = list(m.parameters()), list(twin.parameters())
    opt = ClipAdamEMA(params, ema, lr=1e-3, betas=(0.9, 0.99))
    dose, c = dose.cuda(), c.cuda()
    model_fn = lambda x, times: [m(x, times[0] if objective == "pred_res" else times[1], dose, c)]
    batch, t, noise = [x_start.cuda(), x_input.cuda()], t.cuda(), noise.cuda()
    losses = []
    for k in range(5):
        out = train_step(model_fn, opt, batch, t=t, noise=noise, schedule=_schedule(), objective=objective, loss_type=loss_type)
        assert len(out) == 1 and out[0].shape == () and out[0].is_cuda
        losses.append(float(out[0]))
        if k == 0:
            assert all(torch.equal(e, p.detach()) for e, p in zip(ema, params))
    errs = [abs(a - b) / l64[0] for a, b in zip(losses, l64)]
    gate = max(10 * STEP_GATES[(objective, loss_type)], CAPTURE)
    print(f"[measured] whole step {objective} {loss_type}: losses {losses} float64 {l64} errors {errs} gate {gate:.1e}")
    assert all(np.isfinite(losses))
    assert errs[0] < CAPTURE, errs
    assert all(e < gate for e in errs[1:]), (errs, gate)
    assert all(p.grad is not None and not p.grad.any() for p in params)


# ---- 9. the binding ----------------------------------------------------------------------------------------------------------------
class _DiffusionStandIn(torch.nn.Module):
    """the attributes ResidualDiffusion.p_losses reads (src/DADiff.py:1399-1482), with a two-layer model in the U-Net's place"""

    def __init__(self, objective, n_out, self_condition=False):
        super().__init__()
        sch = _schedule()
        self.register_buffer("alphas_cumsum", sch["alphas_cumsum"])
        self.register_buffer("betas_cumsum", sch["betas_cumsum"])
        self.objective, self.loss_type, self.condition, self.input_condition, self.self_condition = objective, "l1", True, False, \
            self_condition
        self.num_timesteps = T
        self.nets = torch.nn.ModuleList([torch.nn.Conv2d(2, 1, 3, padding=1) for _ in range(n_out)])
        self.calls = 0

        def model(x, times):
            self.calls += 1
            assert x.shape[1] == 2 and len(times) == 2 and times[0].shape == (x.shape[0],)
            return [net(x) * (1 + 1e-3 * times[i][:, None, None, None]) for i, net in enumerate(self.nets)]
        self.model = model


def test_binding():
    """p_losses bound on a stand-in with the reference's attribute names: a list of one loss for pred_res, of two for
    pred_res_noise, equal to the float64 lines; train_step drives it; self_condition=True raises before the model is called"""
    from founddiff_amd import diffusion_train as dt
    _DiffusionStandIn.p_losses = dt.p_losses
    g = torch.Generator().manual_seed(5)
    x0, xi = (torch.rand(2, 1, 8, 12, generator=g) * 2 - 1).cuda(), (torch.rand(2, 1, 8, 12, generator=g) * 2 - 1).cuda()
    t, nz = torch.tensor([0, T - 1]).cuda(), torch.randn(2, 1, 8, 12, generator=g).cuda()
    for objective, n in (("pred_res", 1), ("pred_res_noise", 2)):
        d = _DiffusionStandIn(objective, n).cuda()
        losses = d.p_losses([x0, xi], t, nz)
        assert isinstance(losses, list) and len(losses) == n and all(v.shape == () and v.requires_grad for v in losses)
        ref = _qs_float64(x0.cpu(), xi.cpu(), t.cpu(), nz.cpu(), _schedule(), normalize=False)
        with torch.no_grad():
            outs = d.model(ref["x_in"].float().cuda(), list(ref["times"].float().cuda()))
        targets = [ref["x_res"], nz.double().cpu()]
        errs = {}
        for i in range(n):
            want = (outs[i].double().cpu() - targets[i]).abs().flatten(1).mean(dim=1).mean()
            errs[f"loss{i}"] = abs(float(losses[i]) - float(want)) / float(want)
        _report(f"binding {objective}", errs)
        assert all(e < CAPTURE for e in errs.values()), errs
        opt = dt.ClipAdamEMA(d.nets.parameters(), lr=1e-3)
        before = [p.detach().clone() for p in d.nets.parameters()]
        got = dt.train_step(d, opt, [(x0 + 1) / 2, (xi + 1) / 2], t=t, noise=nz)
        assert len(got) == n and all(not torch.equal(p.detach(), b) for p, b in zip(d.nets.parameters(), before))
    d = _DiffusionStandIn("pred_res", 1, self_condition=True).cuda()
    with pytest.raises(RuntimeError, match="self_condition"):
        d.p_losses([x0, xi], t, nz)
    assert d.calls == 0
