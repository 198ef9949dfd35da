"""founddiff_amd.resample_train (csrc/fd_resample_train.hip) and founddiff_amd.unet_train against float64 torch autograd on the GPU
and against the reference's captured outputs.

Gates, the project's own (tests/test_gpu_resblock_train.py): rel_err (max abs error over the reference's max abs value) < 1e-5 for
forward outputs, < 1e-4 for gradients of activations, < 1e-3 for parameter gradients, < 1e-4 against the reference's captured fp32
module outputs, < 1e-3 for a whole network against its capture.  Every test prints the errors it measured."""
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err

pytestmark = pytest.mark.gpu

ACT, PARAM, OUT, CAPTURE, NET = 1e-4, 1e-3, 1e-5, 1e-4, 1e-3
SENTINEL = -12345.0
CHANNELS = [(32, 32), (64, 32), (32, 64), (128, 64)]
SIZES = [(1, 1), (3, 5), (15, 13), (65, 35)]
KERNEL_CASES = [(ch, hw) for ch in CHANNELS for hw in SIZES] + [((512, 256), (3, 5))]
_ids = lambda c: f"{c[0][0]}-{c[0][1]}-{c[1][0]}x{c[1][1]}"


def _ptr(t):
    return None if t is None else t.data_ptr()


def _report(tag, errs):
    print(f"[measured] {tag}: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))


def _errors(got, ref, names):
    errs = {}
    for name in names:
        assert got[name].shape == ref[name].shape, (name, got[name].shape, ref[name].shape)
        errs[name] = rel_err(got[name].cpu(), ref[name].cpu())
    return errs


def _assert_gates(tag, got, ref, gates):
    errs = _errors(got, ref, gates)
    _report(tag, errs)
    for name, gate in gates.items():
        assert errs[name] < gate, f"{tag}: {name} error {errs[name]:.3e} >= {gate:.0e}"


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---- 1. fd_conv_sub2x_f32 through the C ABI ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("case", KERNEL_CASES, ids=_ids)
def test_conv_sub2x(case, with_bias):
    """fd_conv_sub2x_f32 against float64 F.conv_transpose2d(stride 2, padding 1) on the GPU, batch 2: the use as Down's input
    gradient, w2[n][2a+b][r][s][c] = w[c][n][kh(a,r)][kw(b,s)] with no fold.  out is written into a sentinel-filled buffer with a
    guard row behind it; in, w2 and bias must not change."""
    from founddiff_amd import _lib as L
    from founddiff_amd.resample_train import sub2x_weight
    (Cin, Cout), (H, W) = case
    B = 2
    g = torch.Generator().manual_seed(Cin + 7 * Cout + H * W)
    x = torch.randn(B, H, W, Cin, generator=g).cuda()
    w = (torch.randn(Cin, Cout, 4, 4, generator=g) / (4 * Cin) ** 0.5).cuda()
    bias = torch.randn(Cout, generator=g).cuda() if with_bias else None
    ref = F.conv_transpose2d(x.double().permute(0, 3, 1, 2), w.double(), None if bias is None else bias.double(), stride=2,
                             padding=1).permute(0, 2, 3, 1)
    w2 = sub2x_weight(w.transpose(0, 1))
    assert w2.shape == (Cout, 4, 2, 2, Cin)
    x0, w0, b0 = x.clone(), w2.clone(), (None if bias is None else bias.clone())
    n = B * 2 * H * 2 * W
    out = torch.full((n + 1, Cout), SENTINEL, device="cuda")
    L.call("fd_conv_sub2x_f32", _ptr(x), _ptr(w2), _ptr(bias), _ptr(out), B, H, W, Cin, Cout, _stream())
    torch.cuda.synchronize()
    assert bool((out[-1] == SENTINEL).all()), "the guard row behind out was written"
    assert torch.equal(x, x0) and torch.equal(w2, w0) and (bias is None or torch.equal(bias, b0)), "an input was overwritten"
    _assert_gates(f"sub2x {Cin}->{Cout} {H}x{W} bias={with_bias}", dict(out=out[:-1].reshape(B, 2 * H, 2 * W, Cout)), dict(out=ref),
                  dict(out=OUT))


# ---- 2. fd_corr4x4s2_f32 through the C ABI -----------------------------------------------------------------------------------------
def _corr_ref(coarse, fine, dtype):
    """autograd of F.conv2d(stride 2, padding 1) with respect to a zero weight: [P][Q][4][4]"""
    P, Q = coarse.shape[3], fine.shape[3]
    w = torch.zeros(P, Q, 4, 4, device="cuda", dtype=dtype, requires_grad=True)
    ref, = torch.autograd.grad(F.conv2d(fine.to(dtype).permute(0, 3, 1, 2), w, None, stride=2, padding=1), w,
                               coarse.to(dtype).permute(0, 3, 1, 2))
    return ref


def _corr_case(tag, B, H, W, Q, P, seed, gate=PARAM, splits=None):
    """Q -> P is the Down convolution whose weight gradient this is: fine = x (B, 2H, 2W, Q), coarse = dout (B, H, W, P)"""
    from founddiff_amd import _lib as L
    g = torch.Generator().manual_seed(seed)
    coarse, fine = torch.randn(B, H, W, P, generator=g).cuda(), torch.randn(B, 2 * H, 2 * W, Q, generator=g).cuda()
    ref = _corr_ref(coarse, fine, torch.float64)
    c0, f0 = coarse.clone(), fine.clone()
    nws = L.lib().fd_corr4x4s2_ws_floats(B, H, W, P, Q)
    assert nws > 0
    if splits == 1:
        assert nws == 4
    elif splits is not None:
        assert nws >= splits * P * 16 * Q
    ws = torch.full((nws + 64,), SENTINEL, device="cuda")
    gbuf = torch.full((P * 16 * Q + 64,), SENTINEL, device="cuda")
    L.call("fd_corr4x4s2_f32", _ptr(coarse), _ptr(fine), _ptr(gbuf), _ptr(ws), B, H, W, P, Q, _stream())
    torch.cuda.synchronize()
    assert bool((gbuf[P * 16 * Q:] == SENTINEL).all()), "written past g"
    assert bool((ws[nws:] == SENTINEL).all()), "written past the workspace"
    if splits == 1:
        assert bool((ws == SENTINEL).all()), "one split writes g directly"
    assert torch.equal(coarse, c0) and torch.equal(fine, f0), "an input was overwritten"
    got = gbuf[:P * 16 * Q].reshape(P, 4, 4, Q).permute(0, 3, 1, 2)
    if gate is not None:
        _assert_gates(tag, dict(g=got), dict(g=ref), dict(g=gate))
    return got, ref, coarse, fine


@pytest.mark.parametrize("case", KERNEL_CASES, ids=_ids)
def test_corr4x4s2(case):
    """fd_corr4x4s2_f32 against float64 autograd of F.conv2d(stride 2, padding 1) with respect to its weight, batch 2"""
    (Cin, Cout), (H, W) = case
    _corr_case(f"corr {Cin}->{Cout} coarse {H}x{W}", 2, H, W, Cin, Cout, seed=Cin + 3 * Cout + H * W)


@pytest.mark.parametrize("hw", [(1, 1), (1, 257)])
def test_corr_thin_images(hw):
    """64 -> 64 on a coarse 1 x 1 and 1 x 257 grid: the taps that only ever meet padding (rows 0 and 3; for 1 x 1 columns 0 and 3
    too) are zero in the reference and come out as exact zeros"""
    got, ref, _, _ = _corr_case(f"corr 64->64 coarse {hw[0]}x{hw[1]}", 2, hw[0], hw[1], 64, 64, seed=6 + hw[1])
    for t in (0, 3):
        assert not ref[:, :, t].any() and not got[:, :, t].any()
        if hw[1] == 1:
            assert not ref[:, :, :, t].any() and not got[:, :, :, t].any()
    assert bool(got[:, :, 1, 1].any()) and bool(got[:, :, 2, 2].any())


def test_corr_single_tile_writes_directly():
    """32 -> 32, batch 1, coarse 4 x 8: one pixel tile, one split, g written by the first launch and the workspace untouched"""
    _corr_case("corr 32->32 coarse 4x8 direct", 1, 4, 8, 32, 32, seed=8, splits=1)


def test_corr_long_reduction():
    """32 -> 32, batch 1, coarse 128 x 129: K = 16 512 coarse pixels, several splits.  Here alone the gate is the larger of the
    project gate and 2 x the error of the float32 torch composition against float64, measured in this test on this GPU (the rule
    of tests/test_gpu_resblock_train.py::test_long_reduction).  Both errors are printed."""
    got, ref, coarse, fine = _corr_case("corr long", 1, 128, 129, 32, 32, seed=9, gate=None, splits=2)
    e32 = rel_err(_corr_ref(coarse, fine, torch.float32).cpu(), ref.cpu())
    e = rel_err(got.cpu(), ref.cpu())
    _report("corr long, float32 torch", dict(g=e32))
    _report("corr long, kernel", dict(g=e))
    lim = max(PARAM, 2 * e32)
    assert e < lim, f"g: error {e:.3e} >= {lim:.3e} (project gate {PARAM:.0e}, float32 torch {e32:.3e})"


# ---- 3. the three functions against float64 --------------------------------------------------------------------------------------
NAMES = ("x", "weight", "bias")
GATES = dict(out=OUT, x=ACT, weight=PARAM, bias=PARAM)


def _ref_down(a):
    return F.conv2d(a["x"].permute(0, 3, 1, 2), a["weight"], a["bias"], stride=2, padding=1).permute(0, 2, 3, 1)


def _ref_up(a):
    up = F.interpolate(a["x"].permute(0, 3, 1, 2), scale_factor=2, mode="nearest")
    return F.conv2d(up, a["weight"], a["bias"], padding=1).permute(0, 2, 3, 1)


def _ref_conv3(a):
    return F.conv2d(a["x"].permute(0, 3, 1, 2), a["weight"], a["bias"], padding=1).permute(0, 2, 3, 1)


def _fns():
    from founddiff_amd import resample_train as rt
    return dict(down=(rt.downsample_fn, _ref_down, 4), up=(rt.upsample_fn, _ref_up, 3), conv3=(rt.conv3x3_fn, _ref_conv3, 3))


def _inputs(kind, B, H, W, Cin, Cout, seed):
    """weight = randn / sqrt(taps Cin): out has unit scale; dout for the result's shape"""
    k = 4 if kind == "down" else 3
    g = torch.Generator().manual_seed(seed)
    a = dict(x=torch.randn(B, H, W, Cin, generator=g), weight=torch.randn(Cout, Cin, k, k, generator=g) / (k * k * Cin) ** 0.5,
             bias=0.5 * torch.randn(Cout, generator=g))
    oh, ow = dict(down=(H // 2, W // 2), up=(2 * H, 2 * W), conv3=(H, W))[kind]
    return a, torch.randn(B, oh, ow, Cout, generator=g)


def _grads(fn, inputs, dout, dtype):
    a = {k: v.to("cuda", dtype).requires_grad_() for k, v in inputs.items()}
    out = fn(a)
    r = torch.autograd.grad(out, [a[k] for k in NAMES], dout.to("cuda", dtype))
    return dict(out=out.detach(), **dict(zip(NAMES, r)))


def _fused(kind):
    f = _fns()[kind][0]
    return lambda a: f(a["x"], a["weight"], a["bias"])


FN_CASES = [("down", ch, hw) for ch in [(32, 64), (64, 64), (128, 256)] for hw in [(6, 10), (30, 26)]] + \
           [("up", ch, hw) for ch in [(32, 64), (64, 64), (128, 256), (64, 32), (256, 128)] for hw in [(3, 5), (15, 13)]] + \
           [("up", (512, 256), (3, 5))] + \
           [("conv3", ch, hw) for ch in [(32, 64), (64, 64), (128, 256)] for hw in [(6, 10), (15, 13)]]


@pytest.mark.parametrize("case", FN_CASES, ids=lambda c: f"{c[0]}-{c[1][0]}-{c[1][1]}-{c[2][0]}x{c[2][1]}")
def test_functions_against_float64(case):
    """out and the gradients of x, weight and bias, batch 2, against float64 autograd through the torch composition"""
    kind, (Cin, Cout), (H, W) = case
    inputs, dout = _inputs(kind, 2, H, W, Cin, Cout, seed=Cin + Cout + H)
    ref = _grads(_fns()[kind][1], inputs, dout, torch.float64)
    got = _grads(_fused(kind), inputs, dout, torch.float32)
    _assert_gates(f"{kind} {Cin}->{Cout} {H}x{W}", got, ref, GATES)


def test_conv3x3_reads_a_channel_slice_in_place():
    """x = channels [32, 96) of a wider tensor (ld = 128), 64 -> 32, 15 x 13: the view reaches the kernels as it is, and its gradient
    lands in the slice of the wide tensor's gradient, zeros elsewhere"""
    from founddiff_amd import resample_train as rt
    from founddiff_amd._train import strided
    inputs, dout = _inputs("conv3", 2, 15, 13, 64, 32, seed=77)
    ref = _grads(_ref_conv3, inputs, dout, torch.float64)
    wide = torch.full((2, 15, 13, 128), SENTINEL, device="cuda")
    wide[..., 32:96] = inputs["x"].cuda()
    wide.requires_grad_()
    view = wide[..., 32:96]
    kept, ld, off = strided(view, 64)
    assert kept is view and (ld, off) == (128, 32)
    w, b = inputs["weight"].cuda().requires_grad_(), inputs["bias"].cuda().requires_grad_()
    out = rt.conv3x3_fn(view, w, b)
    r = torch.autograd.grad(out, [wide, w, b], dout.cuda())
    assert not r[0][..., :32].any() and not r[0][..., 96:].any()
    _assert_gates("conv3 wide", dict(out=out.detach(), x=r[0][..., 32:96], weight=r[1], bias=r[2]), ref, GATES)


# ---- 4. the reference's captures ---------------------------------------------------------------------------------------------------
def test_against_the_references_captures(golden):
    """down.* (Downsample 32 -> 64 on 12 x 10) and up.* (Upsample 64 -> 32 on 6 x 5) of tests/golden/modules.npz through
    resample_nhwc on torch modules with the captured weights: forward at 1e-4"""
    from founddiff_amd.resample_train import resample_nhwc
    g = golden("modules")
    nn = torch.nn
    down, up = nn.Conv2d(32, 64, 4, 2, 1), nn.Sequential(nn.Upsample(scale_factor=2, mode="nearest"), nn.Conv2d(64, 32, 3, padding=1))
    for name, m in (("down", down), ("up", up)):
        sd = {k[len(name) + 1:]: v for k, v in g.weights(name + ".").items()}
        m.load_state_dict(sd, strict=True)
        with torch.no_grad():
            got = resample_nhwc(m.cuda(), g[name + ".in"].cuda().permute(0, 2, 3, 1)).permute(0, 3, 1, 2)
        e = rel_err(got.cpu(), g[name + ".out"])
        _report(f"{name} against the capture", dict(out=e))
        assert got.shape == g[name + ".out"].shape and e < CAPTURE, e


# ---- 5. determinism and batch invariance -------------------------------------------------------------------------------------------
_C128 = dict(down=(64, 64), up=(32, 32), conv3=(32, 32))                 # 128 -> 128, coarse 32 x 32


@pytest.fixture(scope="module")
def c128():
    out = {}
    for kind, (H, W) in _C128.items():
        inputs, dout = _inputs(kind, 2, H, W, 128, 128, seed=21)
        out[kind] = (inputs, dout, _grads(_fused(kind), inputs, dout, torch.float32))
    return out


@pytest.mark.parametrize("kind", list(_C128))
def test_determinism(c128, kind):
    """128 -> 128, coarse 32 x 32, batch 2: a second forward + backward gives the same bits of out and every gradient"""
    inputs, dout, got = c128[kind]
    again = _grads(_fused(kind), inputs, dout, torch.float32)
    for name in GATES:
        assert torch.equal(got[name], again[name]), name


@pytest.mark.parametrize("kind", list(_C128))
def test_batch_invariance(c128, kind):
    """slice 1 alone: the same bits of out and of x's gradient as inside the batch of 2"""
    inputs, dout, got = c128[kind]
    alone = _grads(_fused(kind), dict(inputs, x=inputs["x"][1:]), dout[1:], torch.float32)
    assert torch.equal(alone["out"], got["out"][1:])
    assert torch.equal(alone["x"], got["x"][1:])


# ---- 6. memory ---------------------------------------------------------------------------------------------------------------------
def test_memory_below_composition():
    """upsample_fn 128 -> 64, 64 x 64 -> 128 x 128, batch 2: the peak memory of one forward + backward is below that of the torch
    channels-last composition (F.interpolate, F.conv2d) in the same process, which keeps the 4 x up-sampled tensor (the method of
    tests/test_gpu_resblock_train.py::test_memory_below_composition)."""
    from founddiff_amd.resample_train import upsample_fn
    inputs, dout = _inputs("up", 2, 64, 64, 128, 64, seed=31)
    a = {k: v.cuda().requires_grad_() for k, v in inputs.items()}
    cl = dict(a, x=a["x"].detach().permute(0, 3, 1, 2).requires_grad_())          # NCHW shape, channels-last memory
    dout = dout.cuda()
    dout_cl = dout.permute(0, 3, 1, 2)

    def fused():
        return upsample_fn(a["x"], a["weight"], a["bias"]), dout

    def comp():
        return F.conv2d(F.interpolate(cl["x"], scale_factor=2, mode="nearest"), cl["weight"], cl["bias"], padding=1), dout_cl

    def peak(fn, src):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out, d = fn()
        g = torch.autograd.grad(out, [src[k] for k in NAMES], d)
        del out, g
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    f, c = peak(fused, a), peak(comp, cl)
    act = 2 * 128 * 128 * 64 * 4
    print(f"[measured] peak memory: fused {f / 2 ** 20:.0f} MB ({f / act:.2f} output activations), composition {c / 2 ** 20:.0f} MB "
          f"({c / act:.2f} output activations)")
    assert f < c, (f, c)


# ---- 7. the whole trunk ------------------------------------------------------------------------------------------------------------
def _trunk_spec(mults):
    from founddiff_amd import arch
    return {k: v for k, v in arch.da_unet_spec(64, mults).items() if not k.startswith("dose_encoder.")}


def _sinusoidal_emb64(x, dim):
    """oracle.nets.sinusoidal_emb without its casts to float32"""
    import math
    half = dim // 2
    f = torch.exp(torch.arange(half, dtype=x.dtype) * -(math.log(10000) / (half - 1)))
    a = x[:, None] * f[None, :]
    return torch.cat((a.sin(), a.cos()), dim=-1)


def test_trunk_gradients_against_float64(monkeypatch):
    """UnetTrunk(64, (1, 2)) -- one Down, one Up and both plain convolutions -- with synthetic weights, the adaLN-Zero layers
    re-randomised so that both Mamba branches carry gradient; x (2, 2, 16, 16), random dose_embedding and c (normalised).  out, the
    gradient of x and every parameter's gradient against float64 autograd through oracle.nets.da_unet with the torch scan, pe
    built in float64 from the same parameters by da_unet_cond's three lines.  Gates: 1e-4 for out and dx (the project's capture
    gate: a network accumulates), 1e-3 for parameters.  The oracle runs on the CPU, with its sinusoidal embedding (which casts to
    float32) replaced by the same lines in float64."""
    from founddiff_amd import synth
    from founddiff_amd.unet_train import UnetTrunk
    from oracle import nets
    g = torch.Generator().manual_seed(41)
    sd = synth.synth_state_dict(_trunk_spec((1, 2)), 5)
    for k in sd:
        if "adaLN_modulation.1." in k:
            sd[k] = 0.05 * torch.randn(sd[k].shape, generator=g)
    m = UnetTrunk(64, (1, 2))
    m.load_state_dict(sd, strict=True)
    m = m.cuda()
    x, time = torch.randn(2, 2, 16, 16, generator=g), torch.tensor([700.0, 20.0])
    dose = torch.randn(2, 1024, generator=g)
    dose = dose / dose.norm(dim=-1, keepdim=True)
    c = F.normalize(torch.randn(2, 1, 256, generator=g), dim=-1)
    dout = torch.randn(2, 1, 16, 16, generator=g)
    names = sorted(sd)
    # float64 through the oracle, on the CPU (it builds its constants there)
    monkeypatch.setattr(nets, "sinusoidal_emb", _sinusoidal_emb64)
    sd64 = {k: v.double().requires_grad_() for k, v in sd.items()}
    x64 = x.double().requires_grad_()
    tm = F.linear(F.silu(F.linear(dose.double(), sd64["text_mlp.0.weight"], sd64["text_mlp.0.bias"])),
                  sd64["text_mlp.2.weight"], sd64["text_mlp.2.bias"])
    pe = torch.softmax(tm, dim=1) * sd64["prompt"]
    pe = F.linear(pe, sd64["prompt_mlp.weight"], sd64["prompt_mlp.bias"])
    o64 = nets.da_unet(nets.SD(sd64), x64, time.double(), cond=(c.double(), pe), scan_fn=nets.selective_scan_torch)
    r = torch.autograd.grad(o64, [x64] + [sd64[k] for k in names], dout.double())
    ref = dict(out=o64.detach(), x=r[0], **dict(zip(names, r[1:])))
    xg = x.cuda().requires_grad_()
    o = m(xg, time.cuda(), dose.cuda(), c.cuda())
    params = dict(m.named_parameters())
    assert sorted(params) == names
    r = torch.autograd.grad(o, [xg] + [params[k] for k in names], dout.cuda())
    got = dict(out=o.detach(), x=r[0], **dict(zip(names, r[1:])))
    gates = dict(out=CAPTURE, x=CAPTURE, **{k: PARAM for k in names})
    errs = _errors(got, ref, gates)
    worst = max(names, key=lambda k: errs[k])
    _report("trunk (1, 2)", dict(out=errs["out"], x=errs["x"], **{worst: errs[worst]}))
    assert all(bool(ref[k].any()) for k in names), [k for k in names if not ref[k].any()]
    for name, gate in gates.items():
        assert errs[name] < gate, f"{name}: error {errs[name]:.3e} >= {gate:.0e}"


def test_trunk_against_the_capture(golden):
    """UnetTrunk(64, (1, 2, 4, 8)) with full_arch_64.npz's weights, dose_embedding and c from oracle.nets.dose_encoder on the golden
    input, at t = 999 as tests/test_gpu_e2e.py::test_full_arch_64 runs it: against the reference's unet.out at 1e-3"""
    from founddiff_amd.DADiff import ResidualDiffusion, UnetRes
    from founddiff_amd.unet_train import UnetTrunk
    from oracle import nets
    g = golden("full_arch_64")
    pre = "model.unet0."
    sd = {k[len(pre):]: v for k, v in g.weights(pre).items()}
    m = UnetTrunk(64, (1, 2, 4, 8))
    m.load_state_dict({k: v for k, v in sd.items() if not k.startswith("dose_encoder.")}, strict=True)
    m = m.cuda()
    net = UnetRes(dim=64, dim_mults=(1, 2, 4, 8), num_unet=1, condition=True, objective="pred_res", test_res_or_noise="res",
                  precision="fp32")
    dif = ResidualDiffusion(net, image_size=64, timesteps=1000, sampling_timesteps=2, objective="pred_res", loss_type="l2",
                            condition=True, sum_scale=0.01, test_res_or_noise="res")
    time = (dif.alphas_cumsum[999:1000] * 1000).float().cuda()
    xi = (g["x_input"] * 2 - 1).cuda()
    xt = xi + 0.1 * g["noise0"].cuda()
    with torch.no_grad():
        enc = nets.SD({k: v.cuda() for k, v in sd.items() if k.startswith("dose_encoder.")}, "dose_encoder.")
        dose, ctx = nets.dose_encoder(enc, xi.repeat(1, 3, 1, 1))
        out = m(torch.cat((xt, xi), 1), time, dose, ctx.unsqueeze(1))
    e = rel_err(out.cpu(), g["unet.out"])
    _report("trunk (1, 2, 4, 8) against the capture", dict(out=e))
    assert out.shape == g["unet.out"].shape and e < NET, e


class _Encoder(torch.nn.Module):
    """a stub with the dose encoder's call: (anything, dose_embedding (B, 1024), context_embedding (B, 256))"""

    def __init__(self):
        super().__init__()
        self.register_buffer("pd", torch.randn(1, 1024, generator=torch.Generator().manual_seed(1)))
        self.register_buffer("pc", torch.randn(1, 256, generator=torch.Generator().manual_seed(2)))

    def forward(self, x3):
        s = x3.mean(dim=(1, 2, 3))[:, None]
        return None, F.normalize(self.pd + s, dim=-1), F.normalize(self.pc - s, dim=-1)


class _UnetStandIn(torch.nn.Module):
    """the attributes Unet.forward reads (src/DADiff.py:530-683), built from this project's modules and a stub dose_encoder"""

    def __init__(self, trunk):
        super().__init__()
        self.self_condition = False
        self.dose_encoder = _Encoder()
        for name in ("init_conv", "time_mlp", "text_mlp", "prompt_mlp", "downs", "mid_block", "mid_attn", "ups", "final_res_block",
                     "final_conv"):
            setattr(self, name, getattr(trunk, name))
        self.prompt = trunk.prompt


def test_binding_and_layout(monkeypatch):
    """A stand-in with the reference's attribute names (a stub dose_encoder among them) and forward = unet_forward gives the bits
    of UnetTrunk with the same parameters, and every stage hands over a dense NHWC tensor (the permuted view is_contiguous())"""
    from founddiff_amd import mamba_block_train as mbt, resample_train as rt, resblock_train as rbt, synth, unet_train as ut
    sd = synth.synth_state_dict(_trunk_spec((1, 2)), 6)
    g = torch.Generator().manual_seed(7)
    for k in sd:
        if "adaLN_modulation.1." in k:
            sd[k] = 0.05 * torch.randn(sd[k].shape, generator=g)
    trunk = ut.UnetTrunk(64, (1, 2))
    trunk.load_state_dict(sd, strict=True)
    trunk = trunk.cuda()
    _UnetStandIn.forward = ut.unet_forward
    s = _UnetStandIn(trunk).cuda()
    x, time = torch.randn(2, 2, 16, 16, generator=g).cuda(), torch.tensor([300.0, 5.0]).cuda()
    seen = []

    def spy(mod, name, channel_last):
        real = getattr(mod, name)

        def wrapped(module, x, *a):
            v = x if channel_last else x.permute(0, 2, 3, 1)
            seen.append((name, "in", v.is_contiguous()))
            y = real(module, x, *a)
            seen.append((name, "out", (y if channel_last else y.permute(0, 2, 3, 1)).is_contiguous()))
            return y
        monkeypatch.setattr(ut, name, wrapped)
    spy(mbt, "mamba_block_forward", False)
    spy(rbt, "resnet_block_nhwc", True)
    spy(rt, "resample_nhwc", True)
    with torch.no_grad():
        got = s(x, time)
    assert len(seen) == 2 * (2 * 3 + 2 + 2 * 3 + 1) and all(ok for _, _, ok in seen), [e for e in seen if not e[2]]
    monkeypatch.undo()
    with torch.no_grad():
        _, dose, ctx = s.dose_encoder(x[:, 1:2].repeat(1, 3, 1, 1))
        want = trunk(x, time, dose, ctx.unsqueeze(1))
        again = s(x, time)
    assert got.shape == (2, 1, 16, 16) and torch.equal(got, want) and torch.equal(again, want)
    # one optimiser step through the binding: every trunk parameter gets a gradient
    out = s(x, time)
    out.square().mean().backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in trunk.parameters())
