"""founddiff_amd.resblock_train (csrc/fd_resblock_train.hip) against float64 torch autograd on the GPU and against the reference's
captured outputs.

Gates, the project's own (tests/test_gpu_tattn_train.py): rel_err (max abs error over the reference's max abs value) < 1e-5 for
forward outputs, < 1e-4 for gradients of activations (dx, dh, dres), < 1e-3 for parameter gradients, < 1e-4 against the
reference's captured fp32 outputs.  Every test prints the errors it measured."""
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err

pytestmark = pytest.mark.gpu

ACT, PARAM, OUT = 1e-4, 1e-3, 1e-5
SENTINEL = -12345.0
CHANNELS = [(32, 32), (48, 32), (64, 64), (192, 128)]
SIZES = [(3, 5), (15, 13), (130, 70)]


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


# ---- 1. the GroupNorm + SiLU backward through the C ABI --------------------------------------------------------------------------
@pytest.mark.parametrize("hw", SIZES)
@pytest.mark.parametrize("C", [32, 64, 512])
def test_gn_silu_backward(C, hw):
    """fd_gn_silu_bwd_f32 against float64 autograd through F.group_norm + F.silu on the GPU, batch 2, 8 groups, with mean_rstd
    from float64 statistics of h: dh, dgamma, dbeta, dbias.  dh is written into a sentinel-filled buffer with a guard row behind
    it; dout and h must not change."""
    from founddiff_amd import _lib as L
    H, W = hw
    B, G, n = 2, 8, hw[0] * hw[1]
    g = torch.Generator().manual_seed(C + n)
    h = (0.5 + torch.randn(B, n, C, generator=g) * (0.5 + torch.rand(C, generator=g))).cuda()
    dout = torch.randn(B, n, C, generator=g).cuda()
    gamma, beta = (1 + 0.3 * torch.randn(C, generator=g)).cuda(), (0.3 * torch.randn(C, generator=g)).cuda()
    h64, g64, b64 = (t.double().requires_grad_() for t in (h, gamma, beta))
    out = F.silu(F.group_norm(h64.permute(0, 2, 1), G, g64, b64, 1e-5)).permute(0, 2, 1)
    rdh, rdg, rdb = torch.autograd.grad(out, [h64, g64, b64], dout.double())
    hg = h.double().reshape(B, n, G, C // G)
    mean, var = hg.mean(dim=(1, 3)), hg.var(dim=(1, 3), unbiased=False)
    mr = torch.stack([mean, (var + 1e-5).rsqrt()], dim=-1).float().contiguous()
    h0, d0 = h.clone(), dout.clone()
    dh = torch.full((B * n + 1, C), SENTINEL, device="cuda")
    dg, db, dbias = (torch.full((C,), SENTINEL, device="cuda") for _ in range(3))
    nws = L.lib().fd_gn_silu_bwd_ws_floats(B, n, C, G)
    assert nws > 0
    ws = torch.empty(nws, device="cuda")
    L.call("fd_gn_silu_bwd_f32", _ptr(dout), _ptr(h), _ptr(mr), _ptr(gamma), _ptr(beta), _ptr(dh), _ptr(dg), _ptr(db), _ptr(dbias),
           _ptr(ws), B, n, C, G, _stream())
    torch.cuda.synchronize()
    assert bool((dh[-1] == SENTINEL).all()), "the guard row behind dh was written"
    assert torch.equal(h, h0) and torch.equal(dout, d0), "an input was overwritten"
    got = dict(dh=dh[:-1].reshape(B, n, C), dgamma=dg, dbeta=db, dbias=dbias)
    want = dict(dh=rdh, dgamma=rdg, dbeta=rdb, dbias=rdh.sum(dim=(0, 1)))
    _assert_gates(f"gn_silu_bwd C={C} {H}x{W}", got, want, dict(dh=ACT, dgamma=PARAM, dbeta=PARAM, dbias=PARAM))


# ---- the block: inputs, the float64 reference, the fused function ----------------------------------------------------------------
NAMES = ("x", "weight", "bias", "gn_weight", "gn_bias", "res")
GATES = dict(out=OUT, x=ACT, weight=PARAM, bias=PARAM, gn_weight=PARAM, gn_bias=PARAM, res=ACT)


def _inputs(B, H, W, Cin, Cout, seed, res=True, offset=0.0):
    """weight = randn / sqrt(9 Cin): h has unit scale"""
    g = torch.Generator().manual_seed(seed)
    a = dict(x=torch.randn(B, H, W, Cin, generator=g), weight=torch.randn(Cout, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5,
             bias=offset + 0.1 * torch.randn(Cout, generator=g), gn_weight=1 + 0.3 * torch.randn(Cout, generator=g),
             gn_bias=0.3 * torch.randn(Cout, generator=g))
    if res:
        a["res"] = torch.randn(B, H, W, Cout, generator=g)
    return a, torch.randn(B, H, W, Cout, generator=g)


def _ref(a):
    """the composition the reference runs, on channel-last tensors"""
    h = F.conv2d(a["x"].permute(0, 3, 1, 2), a["weight"], a["bias"], padding=1)
    y = F.silu(F.group_norm(h, 8, a["gn_weight"], a["gn_bias"], 1e-5)).permute(0, 2, 3, 1)
    return y + a["res"] if "res" in a else y


def _fused(a):
    from founddiff_amd.resblock_train import block_core_fn
    return block_core_fn(a["x"], a["weight"], a["bias"], a["gn_weight"], a["gn_bias"], a.get("res"))


def _grads(fn, inputs, dout, dtype):
    a = {k: v.to("cuda", dtype).requires_grad_() for k, v in inputs.items()}
    out = fn(a)
    names = [k for k in NAMES if k in a]
    r = torch.autograd.grad(out, [a[k] for k in names], dout.to("cuda", dtype))
    return dict(out=out.detach(), **dict(zip(names, r)))


def _gates(inputs):
    return {k: v for k, v in GATES.items() if k == "out" or k in inputs}


# ---- 2. statistics under a common offset -----------------------------------------------------------------------------------------
def test_statistics_under_a_common_offset():
    """64 -> 64, 64 x 64, batch 2, bias = 10 + 0.1 randn on an h of unit scale: a common offset of 10 sigma in front of the
    GroupNorm statistics (fp32 partial sums over 64-pixel bands, finalised in double).  out and all six gradients."""
    inputs, dout = _inputs(2, 64, 64, 64, 64, seed=2, offset=10.0)
    ref = _grads(_ref, inputs, dout, torch.float64)
    got = _grads(_fused, inputs, dout, torch.float32)
    _assert_gates("offset 10 sigma", got, ref, _gates(inputs))


# ---- 3. the weight gradient through the C ABI ------------------------------------------------------------------------------------
def _wgrad_case(tag, B, H, W, Cin, Cout, seed, wide=False):
    from founddiff_amd import _lib as L
    g = torch.Generator().manual_seed(seed)
    x, dh = torch.randn(B, H, W, Cin, generator=g).cuda(), torch.randn(B, H, W, Cout, generator=g).cuda()
    w64 = torch.zeros(Cout, Cin, 3, 3, device="cuda", dtype=torch.float64, requires_grad=True)
    ref, = torch.autograd.grad(F.conv2d(x.double().permute(0, 3, 1, 2), w64, None, padding=1), w64, dh.double().permute(0, 3, 1, 2))
    ld, off, xin = Cin, 0, x
    if wide:
        ld, off = Cin + 24, 8
        xin = torch.full((B, H, W, ld), SENTINEL, device="cuda")
        xin[..., off:off + Cin] = x
    x0, d0 = xin.clone(), dh.clone()
    nws = L.lib().fd_conv3x3_wgrad_ws_floats(B, H, W, Cin, Cout)
    assert nws > 0
    ws = torch.empty(nws, device="cuda")
    dw = torch.full((Cout * 9 * Cin + 64,), SENTINEL, device="cuda")
    L.call("fd_conv3x3_wgrad_f32", _ptr(xin), ld, off, _ptr(dh), _ptr(dw), _ptr(ws), B, H, W, Cin, Cout, _stream())
    torch.cuda.synchronize()
    assert bool((dw[Cout * 9 * Cin:] == SENTINEL).all()), "written past dweight"
    assert torch.equal(xin, x0) and torch.equal(dh, d0), "an input was overwritten"
    got = dw[:Cout * 9 * Cin].reshape(Cout, 3, 3, Cin).permute(0, 3, 1, 2)
    _assert_gates(tag, dict(dweight=got), dict(dweight=ref), dict(dweight=PARAM))
    return got, ref


@pytest.mark.parametrize("hw", SIZES)
@pytest.mark.parametrize("ch", CHANNELS, ids=lambda c: f"{c[0]}-{c[1]}")
def test_wgrad(ch, hw):
    """fd_conv3x3_wgrad_f32 against float64 autograd through F.conv2d on the GPU, batch 2"""
    _wgrad_case(f"wgrad {ch[0]}->{ch[1]} {hw[0]}x{hw[1]}", 2, hw[0], hw[1], ch[0], ch[1], seed=ch[0] + hw[0] * hw[1])


def test_wgrad_deep():
    """768 -> 512 at 9 x 7: the widest block of the architecture, no split of the pixels"""
    _wgrad_case("wgrad 768->512 9x7", 2, 9, 7, 768, 512, seed=4)


def test_wgrad_reads_a_channel_slice_in_place():
    """x = channels [8, 8 + Cin) of a sentinel-filled wider tensor (ld = Cin + 24, off = 8), 48 -> 32, 15 x 13"""
    _wgrad_case("wgrad wide 48->32 15x13", 2, 15, 13, 48, 32, seed=5, wide=True)


@pytest.mark.parametrize("hw", [(1, 1), (1, 257)])
def test_wgrad_thin_images(hw):
    """64 -> 64 on a 1 x 1 and a 1 x 257 image: only the centre tap, or the centre row of taps, is non-zero in the reference, and
    the others come out as exact zeros"""
    got, ref = _wgrad_case(f"wgrad 64->64 {hw[0]}x{hw[1]}", 2, hw[0], hw[1], 64, 64, seed=6 + hw[1])
    assert not ref[:, :, 0].any() and not ref[:, :, 2].any() and not got[:, :, 0].any() and not got[:, :, 2].any()
    if hw[1] == 1:
        assert not ref[:, :, 1, 0].any() and not ref[:, :, 1, 2].any() and not got[:, :, 1, 0].any() and not got[:, :, 1, 2].any()
    assert bool(got[:, :, 1, 1].any())


# ---- 4. long reduction ---------------------------------------------------------------------------------------------------------------
def test_long_reduction():
    """32 -> 32, batch 1, 256 x 257: K = 65 792 pixels, several splits.  Here alone each entry's gate is the larger of the
    project gate and 2 x the error of the float32 torch composition against float64, measured in this test on this GPU (the rule
    of test_chan_attn_long_reduction).  Both errors are printed."""
    inputs, dout = _inputs(1, 256, 257, 32, 32, seed=3)
    ref = _grads(_ref, inputs, dout, torch.float64)
    t32 = _grads(_ref, inputs, dout, torch.float32)
    got = _grads(_fused, inputs, dout, torch.float32)
    gates = _gates(inputs)
    e32, e = _errors(t32, ref, gates), _errors(got, ref, gates)
    _report("long, float32 torch", e32)
    _report("long, fused", e)
    for name, gate in gates.items():
        lim = max(gate, 2 * e32[name])
        assert e[name] < lim, f"{name}: error {e[name]:.3e} >= {lim:.3e} (project gate {gate:.0e}, float32 torch {e32[name]:.3e})"


# ---- 5. block_core_fn against float64 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [True, False], ids=["res", "nores"])
@pytest.mark.parametrize("ch", CHANNELS + [(768, 512)], ids=lambda c: f"{c[0]}-{c[1]}")
def test_block_core_against_float64(ch, res):
    """out and all six (five without res) gradients, batch 2, 15 x 13; 768 -> 512 at 9 x 7"""
    H, W = (9, 7) if ch == (768, 512) else (15, 13)
    inputs, dout = _inputs(2, H, W, ch[0], ch[1], seed=ch[0] + int(res), res=res)
    ref = _grads(_ref, inputs, dout, torch.float64)
    got = _grads(_fused, inputs, dout, torch.float32)
    _assert_gates(f"block_core {ch[0]}->{ch[1]} {H}x{W} res={res}", got, ref, _gates(inputs))


def test_block_core_reads_a_channel_slice_in_place():
    """x = channels [8, 8 + 48) of a wider tensor (ld = 72, off = 8), 48 -> 32, 15 x 13: the view reaches the kernels as it is, and
    its gradient lands in the slice of the wide tensor's gradient, zeros elsewhere"""
    from founddiff_amd import resblock_train as rbt
    inputs, dout = _inputs(2, 15, 13, 48, 32, seed=77)
    ref = _grads(_ref, inputs, dout, torch.float64)
    wide = torch.full((2, 15, 13, 72), SENTINEL, device="cuda")
    wide[..., 8:56] = inputs["x"].cuda()
    wide.requires_grad_()
    view = wide[..., 8:56]
    kept, ld, off = rbt._strided(view, 48)
    assert kept is view and (ld, off) == (72, 8)
    a = {k: v.cuda().requires_grad_() for k, v in inputs.items() if k != "x"}
    out = rbt.block_core_fn(view, a["weight"], a["bias"], a["gn_weight"], a["gn_bias"], a["res"])
    names = [k for k in NAMES if k != "x"]
    r = torch.autograd.grad(out, [wide] + [a[k] for k in names], dout.cuda())
    assert not r[0][..., :8].any() and not r[0][..., 56:].any()
    got = dict(out=out.detach(), x=r[0][..., 8:56], **dict(zip(names, r[1:])))
    _assert_gates("block_core wide", got, ref, _gates(inputs))


# ---- 6. the modules against the reference's captures and float64 autograd through the oracle on the CPU -------------------------------
def _module_case(tag, m, sd, ref_fn, inputs, captured):
    """inputs: {name: fp32 CPU tensor}; ref_fn(sd64, **inputs64) the oracle; m(**inputs) the module under test"""
    names = sorted(sd)
    with torch.no_grad():
        got = m(**{k: v.cuda() for k, v in inputs.items()})
    e = rel_err(got.cpu(), captured)
    _report(f"{tag} forward against the capture", dict(out=e))
    assert got.shape == captured.shape and e < 1e-4, e
    dout = torch.randn(captured.shape, generator=torch.Generator().manual_seed(5))
    sd64 = {k: v.double().requires_grad_() for k, v in sd.items()}
    in64 = {k: v.double().requires_grad_() for k, v in inputs.items()}
    o64 = ref_fn(sd64, **in64)
    r = torch.autograd.grad(o64, list(in64.values()) + [sd64[k] for k in names], dout.double(), allow_unused=True)
    ref = dict(out=o64.detach(), **dict(zip(list(in64) + names, r)))
    ing = {k: v.cuda().requires_grad_() for k, v in inputs.items()}
    o = m(**ing)
    params = dict(m.named_parameters())
    assert sorted(params) == names
    r = torch.autograd.grad(o, list(ing.values()) + [params[k] for k in names], dout.cuda(), allow_unused=True)
    got = dict(out=o.detach(), **dict(zip(list(ing) + names, r)))
    used = [k for k in ref if ref[k] is not None]
    assert all(got[k] is not None for k in used)
    _assert_gates(f"{tag} grads", got, ref, dict(out=OUT, **{k: (ACT if k in inputs else PARAM) for k in used if k != "out"}))


@pytest.mark.parametrize("which,dims", [("rb_same", (32, 32)), ("rb_proj", (48, 32))])
def test_resnet_block_module(golden, which, dims):
    """resblock_train.ResnetBlock with the reference's rb_same / rb_proj weights (12 x 10, batch 2): the output against the
    reference's capture, the gradients of x and of every parameter against float64 autograd through oracle.nets.da_resnet_block"""
    from founddiff_amd.resblock_train import ResnetBlock
    from oracle import nets
    g = golden("modules")
    sd = {k[len(which) + 1:]: v for k, v in g.weights(which + ".").items()}
    m = ResnetBlock(*dims)
    m.load_state_dict(sd, strict=True)
    _module_case(which, m.cuda(), sd, lambda s, x: nets.da_resnet_block(nets.SD(s), x), dict(x=g[which + ".in"]), g[which + ".out"])


# ---- 7. determinism and batch invariance ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def c128():
    inputs, dout = _inputs(2, 64, 64, 128, 128, seed=21)
    return inputs, dout, _grads(_fused, inputs, dout, torch.float32)


def test_determinism(c128):
    """128 -> 128, 64 x 64, batch 2: a second forward + backward gives the same bits of out and every gradient"""
    inputs, dout, got = c128
    again = _grads(_fused, inputs, dout, torch.float32)
    for name in GATES:
        assert torch.equal(got[name], again[name]), name


def test_batch_invariance(c128):
    """slice 1 alone: the same bits of out and of x's gradient as inside the batch of 2"""
    inputs, dout, got = c128
    alone = _grads(_fused, dict(inputs, x=inputs["x"][1:], res=inputs["res"][1:]), dout[1:], torch.float32)
    assert torch.equal(alone["out"], got["out"][1:])
    assert torch.equal(alone["x"], got["x"][1:])


# ---- 8. memory ---------------------------------------------------------------------------------------------------------------------
def test_memory_below_composition():
    """64 -> 64, 256 x 256, batch 2, identity residual (res = x): the peak memory of one forward + backward of block_core_fn is
    below that of the torch composition the reference runs (NCHW conv, group_norm, silu, + x) in the same process."""
    inputs, dout = _inputs(2, 256, 256, 64, 64, seed=31, res=False)
    a = {k: v.cuda().requires_grad_() for k, v in inputs.items()}
    nchw = dict(a, x=a["x"].detach().permute(0, 3, 1, 2).contiguous().requires_grad_())
    dout = dout.cuda()
    dout_nchw = dout.permute(0, 3, 1, 2).contiguous()

    def fused():
        return _fused(dict(a, res=a["x"])), dout

    def comp():
        h = F.conv2d(nchw["x"], nchw["weight"], nchw["bias"], padding=1)
        return F.silu(F.group_norm(h, 8, nchw["gn_weight"], nchw["gn_bias"], 1e-5)) + nchw["x"], dout_nchw

    def peak(fn, src):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out, d = fn()
        g = torch.autograd.grad(out, [src[k] for k in NAMES[:5]], d)
        del out, g
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    f, c = peak(fused, a), peak(comp, nchw)
    act = 2 * 256 * 256 * 64 * 4
    print(f"[measured] peak memory: fused {f / 2 ** 20:.0f} MB ({f / act:.2f} activations), composition {c / 2 ** 20:.0f} MB "
          f"({c / act:.2f} activations)")
    assert f < c, (f, c)


# ---- 9. binding and layout -----------------------------------------------------------------------------------------------------------
class _WSConvStandIn(torch.nn.Conv2d):
    pass


class _InnerStandIn(torch.nn.Module):
    def __init__(self, dim, dim_out, groups):
        super().__init__()
        self.proj = _WSConvStandIn(dim, dim_out, 3, padding=1)
        self.norm = torch.nn.GroupNorm(groups, dim_out)
        self.act = torch.nn.SiLU()


class _BlockStandIn(torch.nn.Module):
    """the attributes ResnetBlock.forward reads (src/DADiff.py:397-408), built from torch layers alone"""

    def __init__(self, dim, dim_out, groups=8):
        super().__init__()
        self.block1 = _InnerStandIn(dim, dim_out, groups)
        self.res_conv = torch.nn.Conv2d(dim, dim_out, 1) if dim != dim_out else torch.nn.Identity()


def test_binding_and_layout(monkeypatch):
    """A stand-in with the reference's attribute names and forward bound to resnet_block_forward gives the bits of ResnetBlock
    with the same state dict; a permute view of a dense NHWC tensor is used in place and the result is a permute view of a dense
    NHWC tensor; an NCHW-contiguous input gives the same values; MambaBlock -> ResnetBlock -> Conv2d(4, 2, 1) stays channel-last
    at each hand-over; six Adam steps lower a scalar loss and every parameter gets a gradient; a half-precision module and input
    give a half-precision result and finite half-precision gradients."""
    from founddiff_amd import mamba_block_train as mbt, resblock_train as rbt
    torch.manual_seed(9)
    _BlockStandIn.forward = rbt.resnet_block_forward
    g = torch.Generator().manual_seed(10)
    for dims in ((64, 64), (48, 32)):
        m, s = rbt.ResnetBlock(*dims).cuda(), _BlockStandIn(*dims).cuda()
        s.load_state_dict(m.state_dict(), strict=True)
        x = torch.randn(2, dims[0], 12, 10, generator=g).cuda()
        out = m(x)
        assert out.shape == (2, dims[1], 12, 10) and torch.equal(out, s(x))
        assert out.permute(0, 2, 3, 1).is_contiguous()
        # a permute view of a dense NHWC tensor reaches the kernels as it is
        nhwc = x.permute(0, 2, 3, 1).contiguous()
        seen = []
        real = rbt._strided
        monkeypatch.setattr(rbt, "_strided", lambda t, c: (seen.append(t.data_ptr()), real(t, c))[1])
        out2 = m(nhwc.permute(0, 3, 1, 2))
        monkeypatch.setattr(rbt, "_strided", real)
        assert seen == [nhwc.data_ptr()]
        assert torch.equal(out2, out) and out2.permute(0, 2, 3, 1).is_contiguous()
    # Mamba_block -> ResnetBlock -> the down-sampling convolution: channel-last at each hand-over
    mb, rb, down = mbt.MambaBlock(64, 8, 128).cuda(), rbt.ResnetBlock(64, 64).cuda(), torch.nn.Conv2d(64, 128, 4, 2, 1).cuda()
    with torch.no_grad():
        for p in mb.adaLN_modulation[-1].parameters():
            p.copy_(0.2 * torch.randn_like(p))
    x, c, t = (torch.randn(*shape, generator=g).cuda() for shape in ((2, 12, 10, 64), (2, 1, 256), (2, 128)))
    # in the U-Net a Mamba_block's input is a ResnetBlock's result: a permute view of a dense NHWC tensor.  (An NCHW-contiguous
    # input would stay NCHW through the block's residual adds, which take their first operand's layout.)
    x = x.permute(0, 3, 1, 2)
    y0 = mb(x, c, t)
    assert y0.shape == (2, 64, 12, 10) and y0.permute(0, 2, 3, 1).is_contiguous()
    seen = []
    real = rbt._strided
    monkeypatch.setattr(rbt, "_strided", lambda t, c: (seen.append(t.data_ptr()), real(t, c))[1])
    y1 = rb(y0)
    monkeypatch.setattr(rbt, "_strided", real)
    assert seen == [y0.data_ptr()] and y1.permute(0, 2, 3, 1).is_contiguous()
    y2 = down(y1)
    assert y2.shape == (2, 128, 6, 5) and y2.permute(0, 2, 3, 1).is_contiguous()
    # training
    s = _BlockStandIn(48, 32).cuda()
    x = torch.randn(2, 48, 12, 10, generator=g).cuda()
    target = torch.randn(2, 32, 12, 10, generator=g).cuda()
    opt = torch.optim.Adam(s.parameters(), lr=1e-2)
    losses = []
    for _ in range(6):
        opt.zero_grad()
        loss = ((s(x) - target) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert all(p.grad is not None for p in s.parameters())
    assert losses[-1] < losses[0], losses
    h = rbt.ResnetBlock(48, 32).cuda().half()
    xh = x.half().requires_grad_()
    out = h(xh)
    assert out.dtype == torch.float16 and out.shape == (2, 32, 12, 10)
    ref = (F.silu(F.group_norm(F.conv2d(xh.float(), rbt.ws_weight(h.block1.proj.weight.float(), 1e-3), h.block1.proj.bias.float(),
                                        padding=1), 8, h.block1.norm.weight.float(), h.block1.norm.bias.float()))
           + F.conv2d(xh.float(), h.res_conv.weight.float(), h.res_conv.bias.float()))
    e = rel_err(out.float().cpu(), ref.detach().cpu())
    print(f"[measured] half module against the fp32 composition with WS eps 1e-3: {e:.2e}")
    assert e < 2e-2                 # binary16: 2^-11 per rounding of the weight, the residual and the result
    out.float().sum().backward()
    assert xh.grad.dtype == torch.float16 and bool(torch.isfinite(xh.grad.float()).all())
    for name, p in h.named_parameters():
        assert p.grad is not None and p.grad.dtype == torch.float16 and bool(torch.isfinite(p.grad.float()).all()), name
