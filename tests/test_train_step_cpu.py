"""The training step (founddiff_amd.diffusion_train, csrc/fd_train_step.hip), host side, without a GPU: the C ABI of both builds of
the library, the chunk table, the EMA schedule, the optimiser's state-dict conversion, the argument checks and the scratch of the
new kernels."""
import os
import re
import shutil

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("fd_res_qsample_f32", "fd_res_loss_ws_floats", "fd_res_loss_f32", "fd_scale_dev_f32", "fd_opt_chunk_elems",
               "fd_opt_sumsq_f32", "fd_opt_clip_coef", "fd_opt_adam_ema_f32")


def test_new_entries_are_declared_and_exported():
    """declared in include/founddiff_hip.h, present in _lib's table, exported by both builds of the library"""
    from founddiff_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "founddiff_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b(int|int64_t) " + name + r"\(", hdr), name
        assert name in L.SIGNATURES, name
    for build in (L.BF16, L.F16):
        lib = build.lib()
        for name in NEW_SYMBOLS:
            assert hasattr(lib, name), name


def test_workspace_sizes_and_chunk_size():
    """fd_res_loss_ws_floats: positive multiples of 4 at (2, 512^2) and (1, 1), 0 for B = 0 and npix = 0; the library's chunk is the
    module's"""
    from founddiff_amd import _lib as L, diffusion_train as dt
    for build in (L.BF16, L.F16):
        lib = build.lib()
        for B, npix in ((2, 512 * 512), (1, 1)):
            n = lib.fd_res_loss_ws_floats(B, npix)
            assert n > 0 and n % 4 == 0 and n >= B * ((npix + 8191) // 8192), (B, npix, n)
        assert lib.fd_res_loss_ws_floats(0, 512 * 512) == 0 and lib.fd_res_loss_ws_floats(2, 0) == 0
        assert lib.fd_opt_chunk_elems() == dt.CHUNK == 4096


def test_chunk_table():
    """numels (1, 3, 4096, 4097, 70001): 1, 1, 1, 2 and 18 chunks, offsets multiples of 4096, last lengths 1, 3, 4096, 1, 369, every
    element covered exactly once; a tensor's chunks do not depend on its neighbours"""
    from founddiff_amd.diffusion_train import chunk_table
    numels = (1, 3, 4096, 4097, 70001)
    tab = chunk_table(numels)
    assert tab.shape == (23, 3) and str(tab.dtype) == "int64"
    for i, (n, count, last) in enumerate(zip(numels, (1, 1, 1, 2, 18), (1, 3, 4096, 1, 369))):
        rows = tab[tab[:, 0] == i]
        assert len(rows) == count and rows[-1, 2] == last, (n, rows)
        assert (rows[:, 1] % 4096 == 0).all() and (rows[:-1, 2] == 4096).all()
        covered = torch.zeros(n, dtype=torch.int32)
        for _, off, ln in rows.tolist():
            covered[off:off + ln] += 1
        assert bool((covered == 1).all()), n
        alone = chunk_table([n])
        assert (alone[:, 1:] == rows[:, 1:]).all() and (alone[:, 0] == 0).all()
    assert (tab[:, 0] == sorted(tab[:, 0])).all()
    with pytest.raises(RuntimeError, match="no elements"):
        chunk_table([4, 0])


def test_ema_schedule_known_answers():
    """the first 130 calls with the defaults: nothing unless s0 % 10 == 0, a copy for s0 = 0 ... 100, the first decayed update at
    s0 = 110 with epoch 10 (decay 1 - 11 ** (-2 / 3)), clamped at beta later (s0 = 10 000 -> 0.995)"""
    from founddiff_amd.diffusion_train import ema_schedule
    copied = False
    for s0 in range(130):
        mode, decay = ema_schedule(s0, copied)
        if s0 % 10:
            assert mode == 0, s0
        elif s0 <= 100:
            assert (mode, decay) == (1, 0.0), s0
        else:
            epoch = s0 - 100
            assert mode == 2 and decay == 1 - (1 + epoch) ** (-2 / 3), (s0, mode, decay)
        copied = copied or mode != 0
    assert ema_schedule(110, True) == (2, 1 - 11 ** (-2 / 3))
    assert abs(ema_schedule(110, True)[1] - 0.797820) < 1e-6
    assert ema_schedule(10000, True) == (2, 0.995)
    assert ema_schedule(110, False) == (1, 0.0)                          # never copied: the copy comes first
    assert ema_schedule(4, True, update_every=2, update_after_step=4) == (1, 0.0)
    assert ema_schedule(6, True, update_every=2, update_after_step=4) == (2, 1 - 3 ** (-2 / 3))
    assert ema_schedule(6, True, update_every=2, update_after_step=4, min_value=0.9) == (2, 0.9)


def test_adam_state_dict_round_trip():
    """a CPU torch.optim.Adam after two steps (one parameter without a gradient): its state dict -> (steps, exp_avg, exp_avg_sq)
    -> back with identical tensors and steps, and the result loads into torch.optim.Adam"""
    from founddiff_amd.diffusion_train import adam_state_pack, adam_state_unpack
    g = torch.Generator().manual_seed(0)
    params = [torch.nn.Parameter(torch.randn(s, generator=g)) for s in ((3,), (4, 5), (7,))]
    opt = torch.optim.Adam(params, lr=1e-2, betas=(0.9, 0.99))
    for _ in range(2):
        for p in params[:2]:
            p.grad = torch.randn(p.shape, generator=g)
        opt.step()
    sd = opt.state_dict()
    steps, m, v = adam_state_unpack(sd, 3)
    assert steps == [2, 2, 0] and m[2] is None and v[2] is None
    back = adam_state_pack(steps, m, v, sd["param_groups"][0])
    assert back["param_groups"] == sd["param_groups"] and sorted(back["state"]) == sorted(sd["state"]) == [0, 1]
    for i in (0, 1):
        assert float(back["state"][i]["step"]) == float(sd["state"][i]["step"]) == 2.0
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(back["state"][i][k], sd["state"][i][k])
    other = torch.optim.Adam([torch.nn.Parameter(p.detach().clone()) for p in params], lr=1.0)
    other.load_state_dict(dict(back, ema_step=7))                        # the extra key does not stand in the way
    assert other.param_groups[0]["lr"] == 1e-2 and float(other.state[other.param_groups[0]["params"][1]]["step"]) == 2.0
    with pytest.raises(RuntimeError, match="one param group of 2"):
        adam_state_unpack(sd, 2)


def _raises(match, fn, *args, **kw):
    with pytest.raises(RuntimeError, match=match):
        fn(*args, **kw)


def test_functions_reject_before_cuda_is_initialised():
    """types and dtypes, then shapes, then devices: each with its message, and nothing touches the GPU"""
    from founddiff_amd import diffusion_train as dt
    from founddiff_amd.DADiff import residual_schedule
    was = torch.cuda.is_initialized()
    sch = residual_schedule(1000)
    B = 2
    x0, xi, t = torch.rand(B, 1, 4, 6), torch.rand(B, 1, 4, 6), torch.tensor([0, 999])
    nz = torch.randn(B, 1, 4, 6)
    # q_sample
    _raises("GPU", dt.q_sample, x0, xi, t, sch, nz)
    _raises("GPU", dt.q_sample, x0, xi, t, sch, None, torch.tensor([1, 2]))
    _raises("must be a tensor", dt.q_sample, x0, None, t, sch, nz)
    _raises("must be a tensor", dt.q_sample, x0, xi, [0, 999], sch, nz)
    _raises("float32", dt.q_sample, x0.double(), xi, t, sch, nz)
    _raises("float32", dt.q_sample, x0, xi, t, sch, nz.half())
    _raises("int64", dt.q_sample, x0, xi, t.int(), sch, nz)
    _raises("int64", dt.q_sample, x0, xi, t, sch, None, torch.tensor([1.0, 2.0]))
    _raises("must be a tensor", dt.q_sample, x0, xi, t, sch, None, [1, 2])
    _raises("either noise or slice_seeds", dt.q_sample, x0, xi, t, sch, nz, torch.tensor([1, 2]))
    _raises("schedule must be a dict", dt.q_sample, x0, xi, t, None, nz)
    _raises("inconsistent shapes", dt.q_sample, x0, xi, t, dict(sch, betas_cumsum=sch["betas_cumsum"][:-1]), nz)
    _raises("unsupported shape", dt.q_sample, x0.repeat(1, 2, 1, 1), xi.repeat(1, 2, 1, 1), t, sch)
    _raises("unsupported shape", dt.q_sample, x0[0], xi[0], t, sch)
    _raises("inconsistent shapes", dt.q_sample, x0, xi[:, :, :3], t, sch, nz)
    _raises("inconsistent shapes", dt.q_sample, x0, xi, t[:1], sch, nz)
    _raises("inconsistent shapes", dt.q_sample, x0, xi, t, sch, nz[:1])
    _raises("inconsistent shapes", dt.q_sample, x0, xi, t, sch, None, torch.tensor([1, 2, 3]))
    # residual_loss
    _raises("GPU", dt.residual_loss, x0, xi, "l1")
    _raises("must be a tensor", dt.residual_loss, x0, None, "l1")
    _raises("float32", dt.residual_loss, x0, xi.double(), "l2")
    _raises("invalid loss type", dt.residual_loss, x0, xi, "huber")
    _raises("scale must be a number", dt.residual_loss, x0, xi, "l1", torch.tensor(1.0))
    _raises("inconsistent shapes", dt.residual_loss, x0, xi[:1], "l1")
    # p_losses_fn
    fn = lambda x, times: [x[:, :1]]
    _raises("GPU", dt.p_losses_fn, fn, [x0, xi], t, sch, "pred_res", "l2", nz)
    _raises("callable", dt.p_losses_fn, None, [x0, xi], t, sch)
    _raises("unknown objective", dt.p_losses_fn, fn, [x0, xi], t, sch, "pred_v")
    _raises("invalid loss type", dt.p_losses_fn, fn, [x0, xi], t, sch, "pred_res", "l3")
    _raises(r"\[x_start, x_input\]", dt.p_losses_fn, fn, x0, t, sch)
    _raises(r"\[x_start, x_input\]", dt.p_losses_fn, fn, [x0, xi, xi], t, sch)
    _raises("float32", dt.p_losses_fn, fn, [x0, xi.long()], t, sch)
    _raises("unsupported shape", dt.p_losses_fn, fn, [x0.flatten(1), xi.flatten(1)], t, sch, "pred_res", "l2", nz.flatten(1))
    # ClipAdamEMA
    ps = [torch.nn.Parameter(torch.randn(5)), torch.nn.Parameter(torch.randn(2, 3))]
    _raises("GPU", dt.ClipAdamEMA, ps)
    _raises("iterable of tensors", dt.ClipAdamEMA, ps[0])
    _raises("params is empty", dt.ClipAdamEMA, [])
    _raises("must be a tensor", dt.ClipAdamEMA, [ps[0], None])
    _raises("float32", dt.ClipAdamEMA, [ps[0], torch.randn(3).double()])
    _raises("float32", dt.ClipAdamEMA, ps, [torch.randn(5), torch.randn(2, 3).half()])
    _raises("invalid hyperparameters", dt.ClipAdamEMA, ps, None, -1.0)
    _raises("invalid hyperparameters", dt.ClipAdamEMA, ps, None, 1e-4, (0.9, 1.0))
    _raises("inconsistent shapes", dt.ClipAdamEMA, ps, [torch.randn(5)])
    _raises("inconsistent shapes", dt.ClipAdamEMA, ps, [torch.randn(5), torch.randn(3, 2)])
    _raises("unsupported shape", dt.ClipAdamEMA, [torch.randn(4, 6).t()])
    # train_step
    _raises("must be a ClipAdamEMA", dt.train_step, fn, torch.optim.Adam(ps), [x0, xi], t, nz, None, 0, sch)
    opt = object.__new__(dt.ClipAdamEMA)                                 # an instance that was never constructed: nothing may reach it
    _raises("GPU", dt.train_step, fn, opt, [x0, xi], t, nz, None, 0, sch)
    _raises("GPU", dt.train_step, fn, opt, [x0, xi], None, nz, None, 0, sch)
    _raises("GPU", dt.train_step, fn, opt, [[x0, xi], [x0, xi]], [t, t], [nz, nz], None, 0, sch)
    _raises("lists of 2", dt.train_step, fn, opt, [[x0, xi], [x0, xi]], t, nz, None, 0, sch)
    _raises(r"\[x_start, x_input\]", dt.train_step, fn, opt, x0, t, nz, None, 0, sch)
    _raises("float32", dt.train_step, fn, opt, [x0, xi.double()], t, nz, None, 0, sch)
    _raises("inconsistent shapes", dt.train_step, fn, opt, [x0, xi[:1]], t, nz, None, 0, sch)
    _raises("schedule must be a dict", dt.train_step, fn, opt, [x0, xi], t, nz)
    _raises("ResidualDiffusion or a callable", dt.train_step, 5, opt, [x0, xi], t, nz, None, 0, sch)
    assert torch.cuda.is_initialized() == was


class _Diffusion:
    """the attributes p_losses reads, as the reference names them"""
    objective, loss_type, condition, input_condition, self_condition, num_timesteps = "pred_res", "l1", True, False, False, 1000

    def __init__(self):
        from founddiff_amd.DADiff import residual_schedule
        sch = residual_schedule(1000)
        self.alphas_cumsum, self.betas_cumsum = sch["alphas_cumsum"], sch["betas_cumsum"]
        self.model = lambda x, times: [x[:, :1]]


def test_bound_p_losses_rejects_before_cuda_is_initialised():
    """self_condition, input_condition and condition=False raise, and so does a CPU batch, before anything launches"""
    from founddiff_amd import diffusion_train as dt
    was = torch.cuda.is_initialized()
    _Diffusion.p_losses = dt.p_losses
    x0, xi, t = torch.rand(2, 1, 4, 4), torch.rand(2, 1, 4, 4), torch.tensor([3, 500])
    d = _Diffusion()
    _raises("GPU", d.p_losses, [x0, xi], t, torch.randn(2, 1, 4, 4))
    for attr, match in (("self_condition", "self_condition"), ("input_condition", "input_condition")):
        d = _Diffusion()
        setattr(d, attr, True)
        _raises(match, d.p_losses, [x0, xi], t)
    d = _Diffusion()
    d.condition = False
    _raises("condition=False", d.p_losses, [x0, xi], t)
    d = _Diffusion()
    d.num_timesteps = 500
    _raises("num_timesteps", d.p_losses, [x0, xi], t)
    assert torch.cuda.is_initialized() == was


def test_new_kernels_use_no_scratch():
    """0 bytes of scratch per lane for every kernel of csrc/fd_train_step.hip, in both builds (hipcc's kernel-resource-usage
    remarks, founddiff_amd.build.resources())"""
    if not shutil.which("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    from founddiff_amd import build
    want = {"qsample_kernel": 4, "loss_kernel": 4, "loss_finish_kernel": 1, "scale_dev_kernel": 2, "opt_sumsq_kernel": 1,
            "opt_clip_kernel": 1, "opt_adam_kernel": 1, "partial_sum_kernel": 1}
    for half in ("bf16", "fp16"):
        build.build(half=half)
        tab = build.resources(half).get("fd_train_step.hip")
        assert tab, "no resource remarks beside fd_train_step.hip's object: rebuild with build(force=True)"
        seen = {}
        for name, r in tab.items():
            assert r.get("scratch", 0) == 0, (half, name, r)
            m = re.search("|".join(sorted(want, key=len, reverse=True)), name)
            if m:
                seen[m.group(0)] = seen.get(m.group(0), 0) + 1
        assert seen == want, (seen, want)
