"""GPU parity of the assembled denoiser and samplers (through the drop-in Python API) against
(a) golden vectors captured from the reference and (b) the CPU oracle on the same seeded inputs.
Gate (BASELINE.json north_star): <= 1e-3 relative, fp32 parity mode.  bf16 mode is gated on
drift vs fp32 (L2-relative <= 2e-2, see SURVEY 'Hard parts': reference autocast(bf16) itself
drifts 7.4e-3 L2 / 1.8e-2 max)."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

from conftest import gate2x, rel_err

pytestmark = pytest.mark.gpu
TINY_CLIP = dict(layers=(2, 1, 1, 1), width=16, embed_dim=1024)


def l2rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


def nhwc(x, tdt):
    return x.permute(0, 2, 3, 1).contiguous().to("cuda", tdt)


def nchw(x):
    return x.float().cpu().permute(0, 3, 1, 2).contiguous()


class Bare:
    pass


def bare_engine(mode):
    from founddiff_amd import _lib as L
    from founddiff_amd.engine import DAEngine, _T

    class _B(DAEngine):
        def __init__(self):
            self.mode = mode
            self.dt, self.tdt = _T[mode]
            self.hip = L.F16 if mode == "fp16" else L.BF16
            self.dev = torch.device("cuda")
            self.f32 = dict(device=self.dev, dtype=torch.float32)
            self.buf = {}
    return _B()


@pytest.mark.parametrize("mode,tol", [("fp32", 1e-4), ("bf16", 3e-2)])
@pytest.mark.parametrize("name", ["rb_same", "rb_proj"])
def test_resnet_block(golden, mode, tol, name):
    from founddiff_amd.engine import _Sub
    g = golden("modules")
    e = bare_engine(mode)
    r = e._pack_res(_Sub(g.weights(name + "."), name + "."))
    x = g[name + ".in"]
    B, Cin, H, W = x.shape
    xd = nhwc(x, e.tdt)
    if name == "rb_proj":     # exercise the two-source (concat) path: 48 = 32 + 16
        a, b = xd[..., :32].contiguous(), xd[..., 32:].contiguous()
        out = e.res_block(r, a, 32, b, 16, B, H, W, "t")
    else:
        out = e.res_block(r, xd, Cin, None, 0, B, H, W, "t")
    torch.cuda.synchronize()
    gate2x(f"resnet_block[{name}-{mode}]", rel_err(nchw(out), g[name + ".out"]), tol)


@pytest.mark.parametrize("mode,tol", [("fp32", 1e-4), ("bf16", 3e-2)])
@pytest.mark.parametrize("tag", ["c32", "c64", "odd:c32", "odd:c64"])
def test_mamba_block(golden, mode, tol, tag):
    """Mamba_block on the HIP path against the reference's outputs; the odd:* cases are 9x7 / 5x5 images (the scan's
    pad-to-even / crop path, src/emamba2.py:191-199, 253-260)."""
    from founddiff_amd import _lib as L
    from founddiff_amd.engine import _Sub
    g = golden("modules_odd" if tag.startswith("odd:") else "modules")
    tag0, tag = tag, tag.split(":")[-1]
    p = f"mamba_{tag}."
    e = bare_engine(mode)
    m = e._pack_mamba(_Sub(g.weights(p), p))
    m["mod_off"], m["loc_off"] = 0, 0
    e.mod_total, e.loc_total = 6 * m["C"], m["D"]
    x, c, t = g[p + "x"], g[p + "c"], g[p + "t"]
    B, Cc, H, W = x.shape
    e.mod_all = torch.empty(B, 6 * Cc, device="cuda")
    e.linear(t.cuda(), m.pop("adaln_w").cuda(), m.pop("adaln_b").cuda(), e.mod_all, pre_silu=True)
    e.local_all = torch.empty(B, m["D"], device="cuda")
    e.linear(c.reshape(B, 256).cuda(), m.pop("local_w").cuda(), None, e.local_all, L.ACT_SILU)
    out = e.mamba_block(m, nhwc(x, e.tdt), B, H, W, "t")
    torch.cuda.synchronize()
    gate2x(f"mamba_block[{tag0}-{mode}]", rel_err(nchw(out), g[p + "out"]), tol)


@pytest.mark.parametrize("C_,H,W", [(64, 128, 256), (128, 32, 32)])
def test_tiny_qk_channels_stay_in_fp16_range(C_, H, W):
    """the fused Gram kernels keep q / k as fp16 on chip; a q / k channel whose weights are ~1e-6 would be
    subnormal or zero there and get a garbage direction where the reference's F.normalize (src/DADiff.py:273-274) gives
    a unit vector.  The engine packs q / k rows with per-channel power-of-two scales (DAEngine._qk_prescale), which the
    L2 norm cancels exactly: a block whose q / k weights are scaled by 2^-22 / 2^-9 on some channels must give the
    SAME BITS as the unscaled block (C = 64: pwdw_gram_kernel, C = 128: row-GEMM + dwconv_gram_kernel)."""
    from founddiff_amd import _lib as L, arch, synth
    from founddiff_amd.engine import _Sub
    spec = {}
    arch._mamba(spec, "b.", C_, 4, 256)
    w = synth.synth_state_dict(spec, seed=11)
    w2 = {k: v.clone() for k, v in w.items()}
    for c in (3, C_ - 1, C_ + 5, 2 * C_ - 2):            # two q and two k channels
        w2["b.attn_blk.qkv.weight"][c] *= 2.0 ** -22
        w2["b.attn_blk.qkv_dwconv.weight"][c] *= 2.0 ** -9
    B = 2
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, C_, H, W, generator=g)
    t, c = torch.randn(B, 256, generator=g), torch.randn(B, 256, generator=g)
    outs = []
    for wd in (w, w2):
        e = bare_engine("bf16")
        m = e._pack_mamba(_Sub(wd, "b."))
        m["mod_off"], m["loc_off"] = 0, 0
        e.mod_total, e.loc_total = 6 * C_, m["D"]
        e.mod_all = torch.empty(B, 6 * C_, device="cuda")
        e.linear(t.cuda(), m.pop("adaln_w").cuda(), m.pop("adaln_b").cuda(), e.mod_all, pre_silu=True)
        e.local_all = torch.empty(B, m["D"], device="cuda")
        e.linear(c.cuda(), m.pop("local_w").cuda(), None, e.local_all, L.ACT_SILU)
        assert L.lib().fd_pw_dw3x3_gram_ok(e.dt, C_, H, W) == (C_ == 64)
        assert C_ == 64 or L.lib().fd_dwconv_gram_ok(e.dt, C_, H, W)
        outs.append(e.mamba_block(m, nhwc(x, e.tdt), B, H, W, "t").clone())
    torch.cuda.synchronize()
    assert torch.isfinite(outs[0].float()).all()
    assert torch.equal(outs[0], outs[1])


def _tiny_model(golden, precision, S=10):
    from founddiff_amd.DADiff import ResidualDiffusion, UnetRes, load_weights
    g = golden("e2e_da_tiny")
    net = UnetRes(dim=32, dim_mults=(1, 2), num_unet=1, condition=True, objective="pred_res",
                  test_res_or_noise="res", precision=precision, clip_cfg=TINY_CLIP)
    dif = ResidualDiffusion(net, image_size=64, timesteps=1000, sampling_timesteps=S, objective="pred_res",
                            loss_type="l2", condition=True, sum_scale=0.01, test_res_or_noise="res")
    w = g.weights("model.")
    missing, unexpected = dif.load_state_dict(w, strict=False)
    assert not [k for k in missing if k.startswith("model.")], missing[:5]
    assert not unexpected, unexpected[:5]
    dif = dif.to("cuda")
    dif.init()
    return g, dif


def test_dose_encoder(golden):
    """DA-CLIP visual tower + heads on HIP kernels vs the reference's CLIPIQA outputs."""
    from founddiff_amd.DADiff import Unet
    g = golden("modules")
    w = g.weights("iqa.")
    for mode, tol in (("fp32", 1e-4), ("bf16", 3e-2)):
        u = Unet(32, dim_mults=(1, 2), precision=mode, clip_cfg=TINY_CLIP)
        sd = u.state_dict()
        for k, v in w.items():
            kk = "dose_encoder." + k[len("iqa."):]
            if kk in sd:
                sd[kk] = v
        u.load_state_dict(sd)
        u = u.to("cuda")
        dose, ctx = u.encode_condition(g["iqa.in"].cuda())
        torch.cuda.synchronize()
        assert rel_err(dose.cpu(), g["iqa.dose"]) < tol, mode
        assert rel_err(ctx.cpu(), g["iqa.ctx"]) < tol, mode


def test_unet_and_predictions_fp32(golden):
    g, dif = _tiny_model(golden, "fp32")
    xi = (g["x_input"] * 2 - 1).cuda()
    xt = xi + 0.1 * g["ddim.noise0"].cuda()
    tt = torch.full((2,), 979, dtype=torch.long, device="cuda")
    out = dif.model(torch.cat((xt, xi), 1), [dif.alphas_cumsum[tt] * 1000, dif.betas_cumsum[tt] * 1000])[0]
    assert rel_err(out.cpu(), g["unet.out"]) < 1e-3
    p = dif.model_predictions(xi, xt, tt)
    assert rel_err(p.pred_res.cpu(), g["mp.pred_res"]) < 1e-3
    assert rel_err(p.pred_noise.cpu(), g["mp.pred_noise"]) < 1e-3
    assert rel_err(p.pred_x_start.cpu(), g["mp.x_start"]) < 1e-3
    mean, var, logvar = dif.q_posterior(p.pred_res, p.pred_x_start, xt, tt)
    c = lambda k: getattr(dif, k)[tt].reshape(-1, 1, 1, 1)
    ref = c("posterior_mean_coef1") * xt + c("posterior_mean_coef2") * p.pred_res + c("posterior_mean_coef3") * p.pred_x_start
    assert rel_err(mean.cpu(), ref.cpu()) < 1e-5


@pytest.mark.parametrize("use_graph", [False, True])
def test_ddim_tiny_fp32(golden, use_graph):
    """config 1 (DA path): 64x64, 10-step DDIM, identical x_T -> reference output within 1e-3."""
    g, dif = _tiny_model(golden, "fp32")
    dif.use_graph = use_graph
    imgs = dif.sample([g["x_input"].cuda()], batch_size=2, last=False, noise=g["ddim.noise0"].cuda())
    ref = g["ddim.imgs"]
    assert len(imgs) == ref.shape[0]
    for i, im in enumerate(imgs):
        assert rel_err(im.cpu(), ref[i]) < 1e-3, i
    out = dif.sample([g["x_input"].cuda()], batch_size=2, last=True, noise=g["ddim.noise0"].cuda())
    assert rel_err(out[-1].cpu(), g["ddim.out"]) < 1e-3
    assert torch.equal(out[-1], imgs[-1])          # deterministic, graph or not


def psnr(a, b):
    return float(10 * torch.log10(1.0 / ((a.double() - b.double()) ** 2).mean()))


def test_ddim_tiny_bf16_drift(golden):
    """config 1 in the production mode (bf16 kernels, last step on the fp32 engine) against the REFERENCE's own
    output: the drift gate of SURVEY section 7 (L2 <= 1e-2, >= 45 dB); the pure-bf16 loop (final_fp32_steps=0)
    keeps the looser bound the reference's own autocast(bf16) run sits at (7.4e-3 L2 / 49 dB)."""
    g, dif = _tiny_model(golden, "bf16")
    assert dif.final_fp32_steps == 1
    ref = g["ddim.out"]
    out = dif.sample([g["x_input"].cuda()], batch_size=2, last=True, noise=g["ddim.noise0"].cuda())[-1].cpu()
    assert l2rel(out, ref) < 1e-2 and psnr(out, ref) > 45.0
    again = dif.sample([g["x_input"].cuda()], batch_size=2, last=True, noise=g["ddim.noise0"].cuda())[-1].cpu()
    assert torch.equal(out, again)
    eager = dif.sample([g["x_input"].cuda()], batch_size=2, last=False, noise=g["ddim.noise0"].cuda())[-1].cpu()
    assert torch.equal(out, eager)                     # whole-loop graph == per-step graphs, both engines
    # adaLN vectors of all steps from ONE pass in front of the loop (DAEngine.time_cond_table; the default of the one-slice
    # kernel set): bit for bit the per-step vectors
    if not any(k in os.environ for k in ("FOUNDDIFF_TIME_TABLE", "FOUNDDIFF_LOW_LATENCY")):     # (the default, unless the user's switches say otherwise)
        assert dif.time_table is False
    dif._time_table = "1"
    tab = dif.sample([g["x_input"].cuda()], batch_size=2, last=True, noise=g["ddim.noise0"].cuda())[-1].cpu()
    dif._time_table = "auto"
    assert torch.equal(out, tab)
    dif.final_fp32_steps = 0
    pure = dif.sample([g["x_input"].cuda()], batch_size=2, last=True, noise=g["ddim.noise0"].cuda())[-1].cpu()
    assert l2rel(pure, ref) < 2e-2 and psnr(pure, ref) > 40.0
    assert l2rel(out, ref) < l2rel(pure, ref)


def test_graph_cache_one_entry_per_kind(golden):
    """DAEngine.graphs holds one (key, payload) per kind: a repeated sample() replays the same captured loop, the per-step graph
    of a last=False run does not evict it, _drop_graphs empties the cache and the next call captures again -- same bits throughout."""
    g, dif = _tiny_model(golden, "bf16")
    x, nz = g["x_input"].cuda(), g["ddim.noise0"].cuda()
    eng = dif._eng()
    first = dif.sample([x], batch_size=2, last=True, noise=nz)[-1].clone()
    assert set(eng.graphs) == {"ddim_loop"}
    loop = eng.graphs["ddim_loop"][1]
    dif.sample([x], batch_size=2, last=True, noise=nz)
    assert eng.graphs["ddim_loop"][1] is loop
    dif.sample([x], batch_size=2, last=False, noise=nz)
    assert set(eng.graphs) == {"ddim_loop", "step"} and eng.graphs["ddim_loop"][1] is loop
    third = dif.sample([x], batch_size=2, last=True, noise=nz)[-1]
    assert eng.graphs["ddim_loop"][1] is loop and torch.equal(third, first)
    dif._drop_graphs()
    assert all(e.graphs == {} for e in dif.model.unet0._engine.values()) and len(dif.model.unet0._engine) >= 2
    again = dif.sample([x], batch_size=2, last=True, noise=nz)[-1]
    assert set(eng.graphs) == {"ddim_loop"} and eng.graphs["ddim_loop"][1] is not loop
    assert torch.equal(again, first)


def test_step_forward_refuses_other_buffers(golden):
    """A step graph bakes in the four loop buffers it was captured over: _step_forward with another img raises on the host
    (nothing is launched) instead of replaying over the old one."""
    g, dif = _tiny_model(golden, "fp32")
    x = g["x_input"].cuda()
    dif.sample([x], batch_size=2, last=False, noise=g["ddim.noise0"].cuda())
    eng = dif._eng()
    entry = eng.graphs["step"]
    x_in, img, mo, time_buf = dif._loop_buffers(x * 2 - 1, (2, 1, 64, 64))
    assert [t.data_ptr() for t in entry[1][1]] == [t.data_ptr() for t in (x_in, img, time_buf, mo)]
    before = mo.clone()
    with pytest.raises(RuntimeError, match="captured over other buffers"):
        dif._step_forward(x_in, img.clone(), time_buf, mo, eng)
    torch.cuda.synchronize()
    assert eng.graphs["step"] is entry and torch.equal(mo, before)


def test_concurrent_half_batches_bitwise(golden):
    """ResidualDiffusion.sample runs a batch >= 8 as two half-batches on two HIP streams (own engines, own captured
    loop graphs): bit-identical to the single-stream run and to itself."""
    g, dif = _tiny_model(golden, "bf16")
    if "FOUNDDIFF_STREAMS" not in os.environ:
        assert dif.streams == 2                        # the default
    dif.streams = 2
    x = g["x_input"].cuda().repeat(4, 1, 1, 1) * torch.linspace(0.7, 1.0, 8, device="cuda").view(8, 1, 1, 1)
    nz = torch.randn(8, 1, 64, 64, generator=torch.Generator().manual_seed(2)).cuda()
    a = dif.sample([x], batch_size=8, noise=nz)
    b = dif.sample([x], batch_size=8, noise=nz)
    dif.streams = 1
    c = dif.sample([x], batch_size=8, noise=nz)
    assert len(a) == 2 and a[-1].shape == (8, 1, 64, 64)
    assert torch.equal(a[-1], b[-1]) and torch.equal(a[-1], c[-1]) and torch.equal(a[0], c[0])


def test_hybrid_forward_stage_split():
    """DAEngine.forward_hybrid: (i) with two engines of the SAME precision it is the plain forward, bit for bit, for
    every split (the stage methods, the two skip stacks and the level boundary are consistent); (ii) fp32 outside /
    bf16 inside lies between the two pure engines; (iii) fd_cast round-trips."""
    from founddiff_amd import _lib as L, arch, synth
    from founddiff_amd.engine import DAEngine
    spec = arch.da_unet_spec(32, (1, 2, 4), prefix="", clip=TINY_CLIP)
    w = synth.synth_state_dict(spec, seed=1)
    g = torch.Generator().manual_seed(9)
    x_in = (torch.rand(2, 1, 64, 64, generator=g) * 2 - 1).cuda()
    x_t = (x_in + 0.1 * torch.randn(2, 1, 64, 64, generator=g).cuda()).contiguous()
    tb = torch.full((2,), 300.0, device="cuda")
    a32, b32, c16 = DAEngine(w, "", "cuda", "fp32"), DAEngine(w, "", "cuda", "fp32"), DAEngine(w, "", "cuda", "bf16")
    for e in (a32, b32, c16):
        e.encode_condition(x_in)
    ref = a32.forward(x_t, x_in, tb).clone()
    for k in (1, 2):
        assert torch.equal(a32.forward_hybrid(b32, x_t, x_in, tb, outer_levels=k), ref), k
    low = c16.forward(x_t, x_in, tb).clone()
    hyb = a32.forward_hybrid(c16, x_t, x_in, tb, outer_levels=1).clone()
    assert l2rel(hyb.cpu(), ref.cpu()) < l2rel(low.cpu(), ref.cpu()) < 5e-2
    v = torch.randn(4096, generator=g).cuda()
    h = torch.empty(4096, device="cuda", dtype=torch.bfloat16)
    back = torch.empty(4096, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    L.call("fd_cast", L.FD_F32, v.data_ptr(), L.FD_BF16, h.data_ptr(), 4096, st)
    L.call("fd_cast", L.FD_BF16, h.data_ptr(), L.FD_F32, back.data_ptr(), 4096, st)
    assert torch.equal(h, v.to(torch.bfloat16)) and torch.equal(back, v.to(torch.bfloat16).float())


def test_p_sample_loop_tiny_fp32(golden):
    """a6: the ancestral loop DRIVER (src/DADiff.py:1233-1273), all 1000 steps of config 1's model through
    p_sample_loop itself; the first 20 steps and x_T against the reference's goldens (noise supplied per step)."""
    g, dif = _tiny_model(golden, "fp32", S=1000)
    assert not dif.is_ddim_sampling
    nz = {999 - i: g["anc.noise"][i].cuda() for i in range(20)}
    gen = torch.Generator(device="cuda").manual_seed(0)

    def step_noise(t):
        return nz[t] if t in nz else torch.randn((2, 1, 64, 64), device="cuda", generator=gen)
    outs = dif.sample([g["x_input"].cuda()], batch_size=2, last=False, noise=g["ddim.noise0"].cuda(), step_noise=step_noise)
    assert len(outs) == 1001
    xi = g["x_input"] * 2 - 1
    assert rel_err(outs[0].cpu() * 2 - 1, xi + 0.1 * g["ddim.noise0"]) < 1e-5
    for i in range(20):
        assert rel_err(outs[1 + i].cpu() * 2 - 1, g["anc.imgs"][i]) < 1e-3, i
    fin = outs[-1]
    assert torch.isfinite(fin).all() and float(fin.min()) >= 0.0 and float(fin.max()) <= 1.0
    # last=True returns [x_T, final] and equals the last=False run given the same noise stream
    gen.manual_seed(0)
    two = dif.sample([g["x_input"].cuda()], batch_size=2, last=True, noise=g["ddim.noise0"].cuda(), step_noise=step_noise)
    assert len(two) == 2 and torch.equal(two[-1], fin)


def test_p_sample_loop_tiny_bf16_tail(golden):
    """The ancestral driver in the production mode: 1000 bf16 steps of config 1's model whose last step (t = 0) runs
    on the fp32 engine, per-step graphs for both engines; against the fp32 loop on the same noise stream.  Unlike
    DDIM, the posterior mean carries x_t forward with weight coef1 ~ 1, so the rounding of 999 bf16 steps accumulates
    in the image: 3.4e-2 L2 measured (the gate is a regression bound, not a parity claim)."""
    noises = {}

    def run(prec):
        g, dif = _tiny_model(golden, prec, S=1000)
        gen = torch.Generator(device="cuda").manual_seed(1)

        def step_noise(t):
            if t not in noises:
                noises[t] = torch.randn((2, 1, 64, 64), device="cuda", generator=gen)
            return noises[t]
        return dif, dif.sample([g["x_input"].cuda()], batch_size=2, last=True, noise=g["ddim.noise0"].cuda(),
                               step_noise=step_noise)[-1].float().cpu()
    _, ref = run("fp32")
    dif, out = run("bf16")
    # the tail engine was built: fp32 storage, split-bf16 contractions ('fp32s', engine.py)
    assert dif.final_fp32_steps == 1 and "fp32s" in {k[0] for k in dif.model.unet0._engine}
    assert l2rel(out, ref) < 6e-2 and psnr(out, ref) > 35.0
    assert torch.isfinite(out).all()


def test_config2_256_bf16_50step_drift():
    """BASELINE configs[1] (256x256, 50-step DDIM, full architecture + DA-CLIP, bf16) in the production mode (last step:
    levels 0-1 on the fp32 engine) against the fp32 parity engine: L2 <= 1e-2, >= 45 dB (7.3e-3 / 53.4 dB measured;
    5.0e-3 / 56.8 dB with the whole last step in fp32); the pure-bf16 loop is reported with the looser bound it sits
    at (1.2e-2 / 49.3 dB)."""
    from founddiff_amd import synth
    import bench
    dev = torch.device("cuda")
    _, ld = synth.ct_phantom(2, 256, seed=10)
    x = torch.from_numpy(ld).to(dev)
    nz = torch.randn(2, 1, 256, 256, generator=torch.Generator().manual_seed(7)).to(dev)
    outs = {}
    for tag, prec, k in (("fp32", "fp32", 0), ("prod", "bf16", 1), ("pure", "bf16", 0)):
        dif, _ = bench.build_model(dev, 256, 50, prec)
        dif.final_fp32_steps = k
        outs[tag] = dif.sample([x], batch_size=2, noise=nz)[-1].float().cpu()
        del dif
        torch.cuda.empty_cache()
    assert l2rel(outs["prod"], outs["fp32"]) < 1e-2 and psnr(outs["prod"], outs["fp32"]) > 45.0
    assert l2rel(outs["pure"], outs["fp32"]) < 2e-2 and psnr(outs["pure"], outs["fp32"]) > 45.0


def test_config3_512_bf16_50step_drift():
    """BASELINE configs[2], the benchmarked workload itself (512x512, 50 steps): production mode vs the fp32 engine,
    L2 <= 1e-2 and >= 45 dB (7.0e-3 / 53.8 dB measured; whole last step in fp32 4.6e-3 / 57.5 dB; pure bf16
    1.1e-2 / 49.8 dB)."""
    from founddiff_amd import synth
    import bench
    dev = torch.device("cuda")
    _, ld = synth.ct_phantom(2, 512, seed=10)
    x = torch.from_numpy(ld).to(dev)
    nz = torch.randn(2, 1, 512, 512, generator=torch.Generator().manual_seed(7)).to(dev)
    outs = {}
    for tag, prec, k, lv in (("fp32", "fp32", 0, 0), ("prod", "bf16", 1, None), ("full", "bf16", 1, 0), ("pure", "bf16", 0, 0)):
        dif, _ = bench.build_model(dev, 512, 50, prec)
        dif.final_fp32_steps = k
        if lv is not None:
            dif.final_outer_levels = lv
        else:
            assert dif.final_outer_levels == 2 and dif.final_fp32_steps == 1          # the defaults ARE the bench mode
        outs[tag] = dif.sample([x], batch_size=2, noise=nz)[-1].float().cpu()
        del dif
        torch.cuda.empty_cache()
    assert l2rel(outs["prod"], outs["fp32"]) < 1e-2 and psnr(outs["prod"], outs["fp32"]) > 45.0
    assert l2rel(outs["full"], outs["fp32"]) < 6e-3 and psnr(outs["full"], outs["fp32"]) > 55.0
    assert l2rel(outs["pure"], outs["fp32"]) < 2e-2 and psnr(outs["pure"], outs["fp32"]) > 45.0


def test_config5_512_fp8_weights_25step_drift():
    """BASELINE configs[4] (512x512, 25-step DDIM, fp8 weights on the fp8 MFMA): e4m3 weights + e4m3-converted halo in
    every 3x3 conv whose K axis splits into 128-channel slabs (kernel id 12), bf16 elsewhere, last step on the bf16
    engine.  Gated on drift against the fp32 engine like the bf16 mode, with the bound e4m3's 3 mantissa bits allow:
    L2 <= 6e-2, >= 37 dB (3.7e-2 / 40.2 dB measured; 6.7e-2 / 35.0 dB without the bf16 last step)."""
    from founddiff_amd import synth
    import bench
    dev = torch.device("cuda")
    _, ld = synth.ct_phantom(2, 512, seed=10)
    x = torch.from_numpy(ld).to(dev)
    nz = torch.randn(2, 1, 512, 512, generator=torch.Generator().manual_seed(7)).to(dev)
    outs = {}
    for prec in ("fp32", "fp8"):
        dif, _ = bench.build_model(dev, 512, 25, prec)
        outs[prec] = dif.sample([x], batch_size=2, noise=nz)[-1].float().cpu()
        if prec == "fp8":
            eng = dif._eng()
            n8 = sum(1 for cw in [r["conv"] for r in [d["res"] for d in eng.downs] + [eng.mid_res] + [u["res"] for u in eng.ups]
                                  + [eng.final_res]] if cw.w8 is not None)
            assert eng.mode == "fp8" and n8 >= 6          # d2r, d3r, midr, u0r, u1r, u3r, finr carry e4m3 weights
            again = dif.sample([x], batch_size=2, noise=nz)[-1].float().cpu()
            assert torch.equal(again, outs[prec])
        del dif
        torch.cuda.empty_cache()
    assert l2rel(outs["fp8"], outs["fp32"]) < 6e-2 and psnr(outs["fp8"], outs["fp32"]) > 37.0


def test_config4_512_ancestral_bf16_properties():
    """BASELINE configs[3] geometry (512x512, 1000-step ancestral, full architecture, bf16): the first three steps of
    the loop through p_sample -- deterministic, finite, batch-invariant (what sharding 64 slices over 8 GPUs relies
    on), and the t = 0 step returns x_start."""
    import bench
    from founddiff_amd import synth
    dev = torch.device("cuda")
    dif, _ = bench.build_model(dev, 512, 1000, "bf16")
    assert not dif.is_ddim_sampling
    _, ld = synth.ct_phantom(2, 512, seed=10)
    xi = torch.from_numpy(ld).to(dev) * 2 - 1
    g = torch.Generator().manual_seed(3)
    x_t = xi + 0.1 * torch.randn(2, 1, 512, 512, generator=g).to(dev)
    nzs = [torch.randn(2, 1, 512, 512, generator=g).to(dev) for _ in range(3)]

    def run(sl):
        img = x_t[sl].clone()
        for i, t in enumerate((999, 998, 997)):
            img, xs = dif.p_sample(xi[sl], img, t, noise=nzs[i][sl], reuse_condition=i > 0)
        return img, xs
    a, xs = run(slice(0, 2))
    b, _ = run(slice(0, 2))
    assert torch.equal(a, b) and torch.isfinite(a).all() and float(xs.abs().max()) <= 1.0
    s0, _ = run(slice(0, 1))
    s1, _ = run(slice(1, 2))
    assert torch.equal(a[0:1], s0) and torch.equal(a[1:2], s1)
    img0, xs0 = dif.p_sample(xi, a, 0)
    assert torch.equal(img0, xs0)                       # coef3 = 1, coef1 = coef2 = 0, no noise at t = 0


def test_config4_512_full_length_ancestral_keyed():
    """BASELINE configs[3], one GPU's share at full length: the 1000-step ancestral p_sample_loop at 512x512 (full
    architecture, bf16 production mode: graph chunks of 37 steps + the tail step on the higher-precision engine) with
    the per-slice keyed step noise.  Size-independent properties: finite, in [0, 1], run-to-run bitwise, and a slice's
    result is the same in a batch of 2 and alone (what sharding 64 slices over 8 ranks relies on)."""
    import bench
    from founddiff_amd import synth
    dev = torch.device("cuda")
    dif, _ = bench.build_model(dev, 512, 1000, "bf16")
    assert not dif.is_ddim_sampling and dif.final_fp32_steps == 1
    _, ld = synth.ct_phantom(2, 512, seed=10)
    x = torch.from_numpy(ld).to(dev)
    seeds = torch.tensor([64007, 64008])
    a = dif.sample([x], batch_size=2, slice_seeds=seeds)[-1]
    assert dif._anc_steps_run == 1000
    assert torch.isfinite(a).all() and float(a.min()) >= 0.0 and float(a.max()) <= 1.0
    one = dif.sample([x[1:2]], batch_size=1, slice_seeds=seeds[1:2])[-1]
    assert torch.equal(one, a[1:2])
    # the image is a denoised version of its input, not noise: closer to the clean phantom's scale than x_T was
    assert float((a - x).abs().mean()) < 0.2


def test_ancestral_steps_fp32(golden):
    g, dif = _tiny_model(golden, "fp32", S=1000)
    xi = (g["x_input"] * 2 - 1).cuda()
    img = xi + 0.1 * g["ddim.noise0"].cuda()
    for i, t in enumerate(range(999, 979, -1)):
        img, xs = dif.p_sample(xi, img, t, noise=g["anc.noise"][i].cuda(), reuse_condition=i > 0)
        assert rel_err(img.cpu(), g["anc.imgs"][i]) < 1e-3, t
    xt = xi + 0.1 * g["ddim.noise0"].cuda()
    img0, xs0 = dif.p_sample(xi, xt, 0)
    assert rel_err(img0.cpu(), g["anc.t0_img"]) < 1e-3
    assert rel_err(xs0.cpu(), g["anc.t0_xstart"]) < 1e-3


def test_full_arch_64(golden):
    """The shipped architecture (dim 64, mults 1-2-4-8, RN50 DA-CLIP) at 64x64 vs the reference."""
    import os
    from conftest import GOLDEN
    if not os.path.exists(os.path.join(GOLDEN, "full_arch_64.npz")):
        pytest.skip("full_arch_64.npz not generated")
    from founddiff_amd.DADiff import ResidualDiffusion, UnetRes, load_weights
    g = golden("full_arch_64")
    net = UnetRes(dim=64, dim_mults=(1, 2, 4, 8), num_unet=1, condition=True, objective="pred_res",
                  test_res_or_noise="res", precision="fp32")
    dif = ResidualDiffusion(net, image_size=64, timesteps=1000, sampling_timesteps=2, objective="pred_res",
                            loss_type="l2", condition=True, sum_scale=0.01, test_res_or_noise="res")
    missing, unexpected = dif.load_state_dict(g.weights("model."), strict=False)
    assert not [k for k in missing if k.startswith("model.")] and not unexpected
    dif = dif.to("cuda")
    dif.init()
    xi = (g["x_input"] * 2 - 1).cuda()
    xt = xi + 0.1 * g["noise0"].cuda()
    tt = torch.full((1,), 999, dtype=torch.long, device="cuda")
    out = dif.model(torch.cat((xt, xi), 1), [dif.alphas_cumsum[tt] * 1000, dif.betas_cumsum[tt] * 1000])[0]
    assert rel_err(out.cpu(), g["unet.out"]) < 1e-3
    res = dif.sample([g["x_input"].cuda()], batch_size=1, last=True, noise=g["noise0"].cuda())
    assert rel_err(res[-1].cpu(), g["ddim2.out"]) < 1e-3
    net.unet0.precision = "bf16"
    res16 = dif.sample([g["x_input"].cuda()], batch_size=1, last=True, noise=g["noise0"].cuda())
    # production mode: of the two steps, the second runs levels 0-1 on the fp32 engine (2-step DDIM jumps from t = 999
    # straight to x_start: the bf16 first step weighs more than in a 50-step run); whole second step in fp32: <= 1e-2
    assert l2rel(res16[-1].cpu(), g["ddim2.out"]) < 2e-2
    dif.final_outer_levels = 0
    res16f = dif.sample([g["x_input"].cuda()], batch_size=1, last=True, noise=g["noise0"].cuda())
    assert l2rel(res16f[-1].cpu(), g["ddim2.out"]) < 1e-2


def test_vs_oracle_random_256(golden):
    """Full architecture at 256x256 (config 2 geometry), 2 DDIM steps: HIP fp32 vs the CPU oracle."""
    from founddiff_amd import arch, synth
    from founddiff_amd.DADiff import ResidualDiffusion, UnetRes, load_weights
    from oracle import sampler
    spec = arch.da_unet_spec(64, (1, 2, 4, 8), prefix="model.unet0.")
    w = synth.synth_state_dict(spec, seed=3)
    net = UnetRes(dim=64, dim_mults=(1, 2, 4, 8), num_unet=1, condition=True, objective="pred_res",
                  test_res_or_noise="res", precision="fp32")
    dif = ResidualDiffusion(net, image_size=256, timesteps=1000, sampling_timesteps=2, objective="pred_res",
                            loss_type="l2", condition=True, sum_scale=0.01, test_res_or_noise="res")
    load_weights(dif, w)
    dif = dif.to("cuda")
    dif.init()
    _, ld = synth.ct_phantom(1, 256, seed=10)
    x_in = torch.from_numpy(ld)
    noise = torch.randn(1, 1, 256, 256, generator=torch.Generator().manual_seed(10))
    out = dif.sample([x_in.cuda()], batch_size=1, noise=noise.cuda())
    orc = sampler.ResidualOracle(w, prefix="model.unet0.", sampling_timesteps=2)
    ref = orc.sample(x_in, noise)
    assert rel_err(out[-1].cpu(), ref[-1]) < 1e-3


def test_properties_512_bf16():
    """BASELINE config 3 geometry (512x512, full arch, bf16): size-independent properties --
    run-to-run bitwise determinism, batch invariance (slices are independent: a slice's result
    does not depend on what else is in the batch -> sharding over GPUs cannot change it),
    finite and in range."""
    from founddiff_amd import arch, synth
    from founddiff_amd.DADiff import ResidualDiffusion, UnetRes, load_weights
    spec = arch.da_unet_spec(64, (1, 2, 4, 8), prefix="model.unet0.")
    w = synth.synth_state_dict(spec, seed=0)
    net = UnetRes(dim=64, dim_mults=(1, 2, 4, 8), num_unet=1, condition=True, objective="pred_res",
                  test_res_or_noise="res", precision="bf16")
    dif = ResidualDiffusion(net, image_size=512, timesteps=1000, sampling_timesteps=3, objective="pred_res",
                            loss_type="l2", condition=True, sum_scale=0.01, test_res_or_noise="res")
    load_weights(dif, w)
    dif = dif.to("cuda")
    dif.init()
    _, ld = synth.ct_phantom(2, 512, seed=10)
    x = torch.from_numpy(ld).cuda()
    nz = torch.randn(2, 1, 512, 512, generator=torch.Generator().manual_seed(1)).cuda()
    a = dif.sample([x], batch_size=2, noise=nz)[-1]
    b = dif.sample([x], batch_size=2, noise=nz)[-1]
    assert torch.equal(a, b)
    assert torch.isfinite(a).all() and float(a.min()) >= 0.0 and float(a.max()) <= 1.0
    s0 = dif.sample([x[0:1]], batch_size=1, noise=nz[0:1])[-1]
    s1 = dif.sample([x[1:2]], batch_size=1, noise=nz[1:2])[-1]
    assert torch.equal(a[0:1], s0) and torch.equal(a[1:2], s1)
    # the round-4 dataflow (z and v recomputed where they are consumed, GroupNorm apply fused with the down-sampling
    # convolutions) against the stored-z / stored-v / two-pass sequence of the same engine: v and the skip tensors are bit-identical
    # by construction, z differs by bf16 flips at rounding ties, the fused convolution by its fp32 summation order -- two
    # equally valid bf16 computations whose rounding noise is decorrelated: they differ by about what each differs from the
    # fp32 engine (9.9e-3 here; over the 50-step loop both sit at 6.7-6.8e-3 from fp32, profiles/r04_drift_dataflow.txt)
    eng = dif._eng()
    assert eng.z_recompute == 1 and eng.v_recompute and eng.down_fuse
    eng.z_recompute, eng.v_recompute, eng.down_fuse = 0, False, False
    dif._drop_graphs()
    c = dif.sample([x], batch_size=2, noise=nz)[-1]
    assert not torch.equal(a, c) and l2rel(a.float().cpu(), c.float().cpu()) < 2e-2


def test_keyed_noise_kernels_vs_oracle():
    """fd_keyed_normal (Philox4x32-10 + Box-Muller keyed by (slice seed, t, pixel), fd_sched.hip) against its numpy
    restatement oracle/keyed_noise.py; fd_res_posterior_step_keyed == fd_res_posterior_step fed with that noise."""
    import numpy as np
    from founddiff_amd import _lib as L
    from oracle import keyed_noise as kn
    seeds = torch.tensor([5, (1 << 40) + 17, 123456789012345], dtype=torch.int64, device="cuda")
    B, npix = 3, 64 * 64 + 3                                    # not a multiple of 4: ragged last group
    st = torch.cuda.current_stream().cuda_stream
    for t in (1, 999, 0x7FFFFFFF):
        out = torch.empty(B, npix, device="cuda")
        L.call("fd_keyed_normal", seeds.data_ptr(), t, out.data_ptr(), B, npix, st)
        ref = np.stack([kn.keyed_normal(int(sd), t, npix) for sd in seeds.tolist()])
        assert float((out.cpu() - torch.from_numpy(ref)).abs().max()) < 5e-5
    big = torch.empty(1, 1 << 20, device="cuda")
    L.call("fd_keyed_normal", seeds.data_ptr(), 7, big.data_ptr(), 1, 1 << 20, st)
    assert abs(float(big.mean())) < 5e-3 and abs(float(big.std()) - 1) < 5e-3
    # the keyed posterior step: coefficient row t from the device table, step from the device counter
    T = 50
    g = torch.Generator().manual_seed(3)
    mo, xt, xin = (torch.randn(B, npix, generator=g).cuda() for _ in range(3))
    table = torch.randn(T, 4, generator=g).cuda()
    for t in (17, 0):
        t_dev = torch.tensor([t], dtype=torch.int32, device="cuda")
        o1, x1 = torch.empty_like(mo), torch.empty_like(mo)
        L.call("fd_res_posterior_step_keyed", mo.data_ptr(), xt.data_ptr(), xin.data_ptr(), table.data_ptr(), t_dev.data_ptr(),
               seeds.data_ptr(), o1.data_ptr(), x1.data_ptr(), B, npix, st)
        nz = torch.empty_like(mo)
        L.call("fd_keyed_normal", seeds.data_ptr(), t, nz.data_ptr(), B, npix, st)
        o2, x2 = torch.empty_like(mo), torch.empty_like(mo)
        coef = table[t:t + 1].expand(B, 4).contiguous()
        L.call("fd_res_posterior_step", mo.data_ptr(), xt.data_ptr(), xin.data_ptr(), nz.data_ptr() if t > 0 else None,
               coef.data_ptr(), o2.data_ptr(), x2.data_ptr(), B, npix, st)
        torch.cuda.synchronize()
        assert torch.allclose(o1, o2, rtol=0, atol=1e-6) and torch.equal(x1, x2)
    tb = torch.zeros(B, device="cuda")
    times = torch.arange(T, dtype=torch.float32, device="cuda") * 0.5
    t_dev = torch.tensor([T], dtype=torch.int32, device="cuda")
    L.call("fd_ancestral_begin", t_dev.data_ptr(), times.data_ptr(), tb.data_ptr(), B, st)
    assert int(t_dev.item()) == T - 1 and float(tb[0]) == (T - 1) * 0.5 and float(tb[2]) == (T - 1) * 0.5


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_ancestral_keyed_loop_properties(golden, prec):
    """p_sample_loop with the per-slice keyed step noise (BASELINE configs[3]'s sampler): the graph-chunk path is
    bitwise equal to the eager step-by-step path; a slice's result is a function of (its input, its seed) only --
    not of the batch it sits in, nor of the HIP stream (two concurrent sub-batches at batch 8); other seeds give
    other images; everything finite."""
    T = 1000            # the reference's init() hard-codes 1000 timesteps; sampling_timesteps == timesteps -> p_sample_loop
    g, dif = _tiny_model(golden, prec, S=T)
    assert not dif.is_ddim_sampling
    x = g["x_input"].cuda()
    x8 = torch.cat([x, x.flip(0), x * 0.9, x.flip(-1)], 0)[:8].contiguous()
    seeds = torch.arange(8, dtype=torch.int64) + 1000
    a = dif.sample([x8], batch_size=8, slice_seeds=seeds)[-1]               # two sub-batches of 4 on two streams
    assert torch.isfinite(a).all()
    assert "anc" in dif._eng().graphs
    dif.streams = 1
    b = dif.sample([x8], batch_size=8, slice_seeds=seeds)[-1]               # one stream, graph chunks
    assert torch.equal(a, b)
    three = dif.sample([x8[2:5]], batch_size=3, slice_seeds=seeds[2:5])[-1]
    assert torch.equal(three, a[2:5])
    if prec == "fp32":
        dif.use_graph = False
        c = dif.sample([x8[4:6]], batch_size=2, slice_seeds=seeds[4:6])[-1]     # eager, one step at a time
        assert torch.equal(c, a[4:6])
        dif.use_graph = True
        other = dif.sample([x8[5:6]], batch_size=1, slice_seeds=seeds[5:6] + 1)[-1]
        assert not torch.equal(other, a[5:6])
        # last=False returns every step (eager path): x_T, then T images
        steps = dif.sample([x8[:2]], batch_size=2, last=False, slice_seeds=seeds[:2])
        assert len(steps) == T + 1 and torch.equal(steps[-1], a[:2])


def test_low_latency_kernel_set(golden):
    """DAEngine low_latency (the kernel set Trainer.test(batch_size=1) selects: chunked scans at every level instead
    of the single-pass scan of short sequences): same arithmetic in another summation order -- fp32 within 1e-4 of
    the default set and of the reference golden, batch-invariant within itself."""
    g, dif = _tiny_model(golden, "fp32", S=10)
    x, nz = g["x_input"].cuda(), g["ddim.noise0"].cuda()
    a = dif.sample([x], batch_size=x.shape[0], noise=nz)[-1]
    dif.model.unet0.low_latency = True
    b = dif.sample([x], batch_size=x.shape[0], noise=nz)[-1]
    assert ("fp32", 0, "ll") in dif.model.unet0._engine                     # a second engine, its own graphs
    assert rel_err(b.cpu(), a.cpu()) < 1e-4
    b1 = dif.sample([x[0:1]], batch_size=1, noise=nz[0:1])[-1]
    assert torch.equal(b1, b[0:1])
    # the flag at the C ABI, on a shape the single-pass scan serves (the 64x64 level of the shipped model: d_inner 1024,
    # N = 32, R = 32): both forms agree to summation order, and they ARE two forms (not bitwise equal)
    from founddiff_amd import _lib as L
    B, D, N, R, H, W = 1, 128, 32, 8, 32, 32
    assert L.lib().fd_selective_scan_plan(L.FD_BF16, D, N, R, H, W) == 0
    assert L.lib().fd_selective_scan_plan(L.FD_BF16 | L.FD_OPT_LOW_LATENCY, D, N, R, H, W) == 1
    g = torch.Generator().manual_seed(2)
    xc = (torch.randn(B, H, W, D, generator=g) * 0.5).cuda()
    xdbl = torch.randn(4, B, (H // 2) * (W // 2), R + 2 * N, generator=g).cuda()
    dtw, dtb = (torch.randn(4, D, R, generator=g) * R ** -0.5).cuda(), (torch.randn(4, D, generator=g) * 0.5 - 3).cuda()
    A = -torch.exp(torch.log(torch.arange(1, N + 1).float())[None].repeat(4 * D, 1)).cuda()
    Ds = torch.ones(4 * D).cuda()
    ws = torch.empty(L.lib().fd_scan_ws_floats(B, H, W, D, N), device="cuda")
    ys = []
    for opts in (0, L.FD_OPT_LOW_LATENCY):
        y = torch.empty(B, H, W, D, device="cuda")
        L.call("fd_selective_scan", L.FD_F32 | opts, xc.data_ptr(), xdbl.data_ptr(), dtw.data_ptr(), dtb.data_ptr(), A.data_ptr(),
               Ds.data_ptr(), y.data_ptr(), ws.data_ptr(), B, H, W, D, N, R, torch.cuda.current_stream().cuda_stream)
        ys.append(y)
    torch.cuda.synchronize()
    assert rel_err(ys[1].cpu(), ys[0].cpu()) < 1e-5 and not torch.equal(ys[0], ys[1])


VARIANTS = {   # name -> (num_unet, objective, test_res_or_noise); mirrors tests/golden/make_golden.py
    "pred_noise": (1, "pred_noise", "noise"), "res_noise": (2, "pred_res_noise", "res_noise"),
    "rn_noise": (2, "pred_res_noise", "noise"), "rn_res": (2, "pred_res_noise", "res"),
    "x0_noise": (2, "pred_x0_noise", "res_noise"), "incond": (1, "pred_res", "res"), "incond_mask": (1, "pred_res", "res"),
}


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_objective_variants_fp32(golden, name):
    """the other objectives and the dual-UNet model, HIP path (fp32 mode) against the
    reference's own outputs: model_predictions, every step of a 4-step DDIM, 3 ancestral steps."""
    from founddiff_amd.DADiff import ResidualDiffusion, UnetRes, load_weights
    g = golden("e2e_da_variants")
    nu, obj, tst = VARIANTS[name]
    ic, mask = name.startswith("incond"), name == "incond_mask"
    net = UnetRes(dim=32, dim_mults=(1, 2), num_unet=nu, condition=True, objective=obj, test_res_or_noise=tst,
                  precision="fp32", clip_cfg=TINY_CLIP, input_condition=ic)
    dif = ResidualDiffusion(net, image_size=64, timesteps=1000, sampling_timesteps=4, objective=obj, loss_type="l2",
                            condition=True, sum_scale=0.01, test_res_or_noise=tst, input_condition=ic,
                            input_condition_mask=mask)
    if ic:      # the 3-plane models were generated under their own key namespace
        w = {k.replace("model_ic.", "model.", 1): v for k, v in g.weights("model_ic.").items()}
    else:
        w = {k: v for k, v in g.weights("model.").items() if nu == 2 or not k.startswith("model.unet1.")}
    missing, unexpected = dif.load_state_dict(w, strict=False)
    assert not [k for k in missing if k.startswith("model.")], missing[:5]
    assert not unexpected, unexpected[:5]
    dif = dif.to("cuda")
    dif.init()
    # x_start from a noise prediction divides by one_minus_alphas_cumsum[t] ~ 6.5e-3: UNet-output
    # differences are amplified ~150x in those two variants (same loosening as the oracle test)
    tol = 5e-3 if name in ("pred_noise", "rn_noise") else 1e-3
    x01 = g["x_input"].cuda()
    xi = x01 * 2 - 1
    xt = xi + 0.1 * g["noise0"].cuda()
    tt = torch.full((1,), 979, dtype=torch.long, device="cuda")
    c01 = g["x_cond2"].cuda()
    xc2 = (c01 if mask else c01 * 2 - 1) if ic else 0
    p = dif.model_predictions(xi, xt, tt, xc2)
    assert rel_err(p.pred_res.cpu(), g[name + ".mp.pred_res"]) < tol
    assert rel_err(p.pred_noise.cpu(), g[name + ".mp.pred_noise"]) < 1e-3
    assert rel_err(p.pred_x_start.cpu(), g[name + ".mp.x_start"]) < tol
    outs = dif.sample([x01, c01] if ic else [x01], batch_size=1, last=False, noise=g["noise0"].cuda())
    ref = g[name + ".ddim.imgs"]
    assert len(outs) == ref.shape[0]
    for i, o in enumerate(outs):
        assert rel_err(o.cpu(), ref[i]) < tol, i
    img = xt.clone()
    for i, t in enumerate(range(999, 996, -1)):
        img, _ = dif.p_sample(xi, img, t, xc2, noise=g["anc.noise"][i].cuda())
        assert rel_err(img.cpu(), g[name + ".anc.imgs"][i]) < tol, t


@pytest.mark.parametrize("cfg", [("tiny", 48, 80), ("tiny", 38, 46), ("tiny", 34, 36), ("full", 72, 88)])
def test_odd_sizes_fp32(cfg):
    """Sizes that are not multiples of 16 -- HIP path (fp32 mode) against the CPU oracle on one model_predictions call:
    48 x 80: the RN50 tower ends on a 3 x 5 map that its last stride-2 AvgPool2d floors to 1 x 2 (nn.AvgPool2d
    semantics, src/DACLIP.py:187) and no 3x3 conv meets the halo kernel's tiling; 38 x 46 / 34 x 36 (tiny model) and
    72 x 88 (shipped architecture): the deepest level is 19 x 23 / 17 x 18 / 9 x 11, so the SS2D scan runs the
    reference's pad-to-even / crop path (src/emamba2.py:191-199, 253-260) and every other kernel an odd image."""
    from founddiff_amd import arch, synth
    from founddiff_amd.DADiff import ResidualDiffusion, UnetRes, load_weights
    from oracle import sampler
    kind, H, W = cfg
    dim, mults, clip = (32, (1, 2), TINY_CLIP) if kind == "tiny" else (64, (1, 2, 4, 8), None)
    spec = arch.da_unet_spec(dim, mults, prefix="model.unet0.", **({"clip": clip} if clip else {}))
    w = synth.synth_state_dict(spec, seed=0)
    g = torch.Generator().manual_seed(5)
    x_in = torch.rand(1, 1, H, W, generator=g) * 2 - 1
    x_t = x_in + 0.1 * torch.randn(1, 1, H, W, generator=g)
    tt = torch.full((1,), 700, dtype=torch.long)
    ref = sampler.ResidualOracle(w, prefix="model.unet0.", sampling_timesteps=2).model_predictions(x_in, x_t, tt)
    net = UnetRes(dim=dim, dim_mults=mults, num_unet=1, condition=True, objective="pred_res", test_res_or_noise="res",
                  precision="fp32", clip_cfg=clip)
    dif = ResidualDiffusion(net, image_size=H, timesteps=1000, sampling_timesteps=2, objective="pred_res", loss_type="l2",
                            condition=True, sum_scale=0.01, test_res_or_noise="res")
    load_weights(dif, w)
    dif = dif.to("cuda")
    dif.init()
    p = dif.model_predictions(x_in.cuda(), x_t.cuda(), tt.cuda())
    assert rel_err(p.pred_res.cpu(), ref[0]) < 1e-3
    assert rel_err(p.pred_x_start.cpu(), ref[2]) < 1e-3
    # bf16 kernels on the same odd geometry: drift gate against the fp32 engine's raw output
    net.unet0.precision = "bf16"
    p16 = dif.model_predictions(x_in.cuda(), x_t.cuda(), tt.cuda())
    assert l2rel(p16.pred_res.cpu(), p.pred_res.cpu()) < 3e-2


def test_vs_oracle_512_one_forward():
    """BASELINE configs[2] geometry (512x512, full architecture), ONE model_predictions call.
    fp32 mode against the CPU oracle: the 1e-3 parity gate at the bench size.
    bf16 mode -- the only place every production fast path runs together (fused LN->1x1->depthwise, LDS-DMA
    halo conv, row-GEMM prologues, 256x256 tiles, buffer-addressed scan) -- one forward, so the precision schedule
    of the sampling loops does not apply: (a) against the fp32 engine on a uniform-noise image, L2 <= 1.5e-2
    (1.1e-2 measured at every size from 144x176 to 512x512, tools/oddsize_check.py); (b) against the oracle on the
    CT phantom, L2 <= 4.5e-2 of the raw residual (3.3e-2 .. 3.7e-2 measured over noise seeds; profiles/r02_drift_table.md: 29 % of that
    variance is the bf16 rounding of the weights, the rest is spread evenly over ~100 activation roundings, and
    this seed's final 64 -> 1 projection amplifies the 1.1e-2 relative error of its input threefold) and
    <= 1.2e-2 (8.5e-3 measured) of x_start = clamp(x_in - residual), the quantity the samplers return."""
    from founddiff_amd import arch, synth
    from founddiff_amd.DADiff import ResidualDiffusion, UnetRes, load_weights
    from oracle import sampler
    spec = arch.da_unet_spec(64, (1, 2, 4, 8), prefix="model.unet0.")
    w = synth.synth_state_dict(spec, seed=0)
    _, ld = synth.ct_phantom(1, 512, seed=10)
    x_in = torch.from_numpy(ld) * 2 - 1
    g = torch.Generator().manual_seed(4)
    x_t = x_in + 0.1 * torch.randn(1, 1, 512, 512, generator=g)
    u_in = torch.rand(1, 1, 512, 512, generator=g) * 2 - 1
    u_t = u_in + 0.1 * torch.randn(1, 1, 512, 512, generator=g)
    tt = torch.full((1,), 500, dtype=torch.long)
    torch.set_num_threads(min(32, torch.get_num_threads()))
    ref = sampler.ResidualOracle(w, prefix="model.unet0.", sampling_timesteps=50).model_predictions(x_in, x_t, tt)
    raw = {}
    for prec in ("fp32", "bf16"):
        net = UnetRes(dim=64, dim_mults=(1, 2, 4, 8), num_unet=1, condition=True, objective="pred_res",
                      test_res_or_noise="res", precision=prec)
        dif = ResidualDiffusion(net, image_size=512, timesteps=1000, sampling_timesteps=50, objective="pred_res",
                                loss_type="l2", condition=True, sum_scale=0.01, test_res_or_noise="res")
        load_weights(dif, w)
        dif = dif.to("cuda")
        dif.init()
        p = dif.model_predictions(x_in.cuda(), x_t.cuda(), tt.cuda())
        if prec == "fp32":
            assert rel_err(p.pred_res.cpu(), ref[0]) < 1e-3
            assert rel_err(p.pred_x_start.cpu(), ref[2]) < 1e-3
        else:
            assert l2rel(p.pred_res.cpu(), ref[0]) < 4.5e-2
            assert l2rel(p.pred_x_start.cpu(), ref[2]) < 1.2e-2
        eng = dif._eng()
        eng.encode_condition(u_in.cuda())
        raw[prec] = eng.forward(u_t.cuda().contiguous(), u_in.cuda().contiguous(), torch.full((1,), 500.0, device="cuda")).cpu()
        del dif, net, eng
    assert l2rel(raw["bf16"], raw["fp32"]) < 1.5e-2
