"""founddiff_amd.tattn_train / mamba_block_train (csrc/fd_tattn_train.hip, fd_dwconv3x3_bwd_f32 of csrc/fd_ss2d_train.hip) against
float64 and against the reference's captured outputs.

Gates, the project's own (tests/test_gpu_ss2d_train.py): rel_err (max abs error over the reference's max abs value) < 1e-5 for
forward outputs, < 1e-4 for gradients of activations, < 1e-3 for parameter gradients, < 1e-4 against the reference's captured
fp32 outputs.  dq, dk and dv are gated separately: max|dq| is a few percent of max|dv| at large hw, a joint gate on dqkv would
hide the softmax / normalisation path.

Inputs of the attention tests: q = randn, k = 0.7 q[..., perm] + 0.7 randn with a fixed permutation inside every head (matched
channels have cosine ~ 0.7 at every hw: the softmax is far from uniform and dS carries signal), v = randn, temperature uniform
in [0.5, 4].  Every test prints the errors it measured."""
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err

pytestmark = pytest.mark.gpu

ACT, PARAM, OUT = 1e-4, 1e-3, 1e-5
SENTINEL = -12345.0


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


# ---- 1. the linear depthwise-conv backward through the C ABI --------------------------------------------------------------------
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("hw", [(3, 5), (15, 13), (130, 70)])
@pytest.mark.parametrize("C", [192, 1536])
def test_dwconv_backward(C, hw, bias):
    """fd_dwconv3x3_bwd_f32 against float64 autograd through F.conv2d on the GPU, batch 2: dx written into the first half of a
    sentinel-filled (B, H, W, 2C) tensor whose second half must stay untouched; dout must not change.  The errors are printed."""
    from founddiff_amd import _lib as L
    H, W = hw
    B = 2
    g = torch.Generator().manual_seed(C + H * W)
    x = torch.randn(B, H, W, C, generator=g)
    w = torch.randn(C, 1, 3, 3, generator=g) / 3
    b = 0.1 * torch.randn(C, generator=g) if bias else None
    dout = torch.randn(B, H, W, C, generator=g)
    x64 = x.cuda().double().requires_grad_()
    w64 = w.cuda().double().requires_grad_()
    b64 = b.cuda().double().requires_grad_() if bias else None
    y = F.conv2d(x64.permute(0, 3, 1, 2), w64, b64, padding=1, groups=C).permute(0, 2, 3, 1)
    ref = torch.autograd.grad(y, [x64, w64] + ([b64] if bias else []), dout.cuda().double())
    xd, w9 = x.cuda(), w.reshape(C, 9).t().contiguous().cuda()
    bd = b.cuda() if bias else None
    dd = dout.cuda()
    dx2 = torch.full((B, H, W, 2 * C), SENTINEL, device="cuda")
    dw9, db = torch.empty(9, C, device="cuda"), (torch.empty(C, device="cuda") if bias else None)
    n = L.lib().fd_dwconv3x3_bwd_ws_floats(B, H, W, C)
    assert n > 0
    ws = torch.empty(n, device="cuda")
    L.call("fd_dwconv3x3_bwd_f32", _ptr(xd), C, 0, _ptr(w9), _ptr(bd), _ptr(dd), _ptr(dx2), 2 * C, 0, _ptr(dw9), _ptr(db), _ptr(ws),
           B, H, W, C, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert bool((dx2[..., C:] == SENTINEL).all()), "the other half of dx was written"
    assert torch.equal(dd.cpu(), dout), "dout was overwritten"
    got = dict(dx=dx2[..., :C], dweight=dw9.t().reshape(C, 1, 3, 3))
    want = dict(dx=ref[0], dweight=ref[1])
    gates = dict(dx=ACT, dweight=PARAM)
    if bias:
        got["dbias"], want["dbias"], gates["dbias"] = db, ref[2], PARAM
    _assert_gates(f"dwconv_bwd C={C} {H}x{W} bias={bias}", got, want, gates)


# ---- 2. - 4. the attention core against the reference formula in float64 ------------------------------------------------------------
def _attn_ref(qkv, temperature):
    """src/DADiff.py:267-281 on a channel-last qkv (B, H, W, 3C), heads of 32 channels"""
    B, H, W, C3 = qkv.shape
    C = C3 // 3
    heads = C // 32
    q, k, v = (t.reshape(B, H * W, heads, 32).permute(0, 2, 3, 1) for t in qkv.split(C, dim=-1))
    q, k = F.normalize(q, dim=-1), F.normalize(k, dim=-1)
    attn = ((q @ k.transpose(-2, -1)) * temperature.reshape(heads, 1, 1)).softmax(dim=-1)
    return (attn @ v).permute(0, 3, 1, 2).reshape(B, H, W, C)


def _attn_inputs(B, H, W, C, seed):
    g = torch.Generator().manual_seed(seed)
    perm = torch.tensor([32 * (c // 32) + (5 * (c % 32) + 3) % 32 for c in range(C)])
    q = torch.randn(B, H, W, C, generator=g)
    k = 0.7 * q[..., perm] + 0.7 * torch.randn(B, H, W, C, generator=g)
    v = torch.randn(B, H, W, C, generator=g)
    temperature = 0.5 + 3.5 * torch.rand(C // 32, 1, 1, generator=g)
    return torch.cat([q, k, v], dim=-1), temperature, torch.randn(B, H, W, C, generator=g)


def _attn_grads(fn, qkv, temperature, dout, dtype):
    C = dout.shape[-1]
    a, t = qkv.to("cuda", dtype).requires_grad_(), temperature.to("cuda", dtype).requires_grad_()
    out = fn(a, t)
    da, dt = torch.autograd.grad(out, [a, t], dout.to("cuda", dtype))
    dq, dk, dv = da.split(C, dim=-1)
    return dict(out=out.detach(), dq=dq, dk=dk, dv=dv, dtemperature=dt)


def _fused_attn(a, t):
    from founddiff_amd.tattn_train import chan_attn_fn
    return chan_attn_fn(a, t)


ATTN_GATES = dict(out=OUT, dq=ACT, dk=ACT, dv=ACT, dtemperature=PARAM)


@pytest.mark.parametrize("hw", [(3, 5), (16, 16), (1, 257), (130, 70)])
@pytest.mark.parametrize("C", [64, 128, 512])
def test_chan_attn_against_float64(C, hw):
    """chan_attn_fn against the reference formula in float64 on the GPU, batch 2, image sizes around the Gram block of 256
    pixels.  The errors are printed."""
    H, W = hw
    qkv, temperature, dout = _attn_inputs(2, H, W, C, seed=C + H * W)
    ref = _attn_grads(_attn_ref, qkv, temperature, dout, torch.float64)
    got = _attn_grads(_fused_attn, qkv, temperature, dout, torch.float32)
    _assert_gates(f"chan_attn C={C} {H}x{W}", got, ref, ATTN_GATES)


def test_chan_attn_reads_a_channel_slice_in_place():
    """the same with qkv a view of channels [8, 8 + 3C) of a wider tensor (ld = 3C + 24, off = 8), C = 128, 15 x 13: the view
    reaches the kernels as it is, and its gradient lands in the slice of the wide tensor's gradient"""
    from founddiff_amd import tattn_train as tat
    C = 128
    qkv, temperature, dout = _attn_inputs(2, 15, 13, C, seed=77)
    ref = _attn_grads(_attn_ref, qkv, temperature, dout, torch.float64)
    wide = torch.full((2, 15, 13, 3 * C + 24), SENTINEL, device="cuda")
    wide[..., 8:8 + 3 * C] = qkv.cuda()
    wide.requires_grad_()
    view = wide[..., 8:8 + 3 * C]
    kept, ld, off = tat._strided(view, 3 * C)
    assert kept is view and (ld, off) == (3 * C + 24, 8)
    t = temperature.cuda().requires_grad_()
    out = tat.chan_attn_fn(view, t)
    dwide, dt = torch.autograd.grad(out, [wide, t], dout.cuda())
    assert not dwide[..., :8].any() and not dwide[..., 8 + 3 * C:].any()
    dq, dk, dv = dwide[..., 8:8 + 3 * C].split(C, dim=-1)
    _assert_gates("chan_attn wide", dict(out=out.detach(), dq=dq, dk=dk, dv=dv, dtemperature=dt), ref, ATTN_GATES)


def test_chan_attn_long_reduction():
    """C = 64, batch 1, hw = 256 x 257 = 65 792 pixels: past the 65 536 switch of the Gram block size (1024-pixel blocks).  At
    this length float32 torch itself sits at 1e-5 .. 2e-5 on out against float64, above the forward gate; so here alone each
    entry's gate is the larger of the project gate and 2 x the error of the float32 torch composition against float64, measured
    in this test on this GPU (the project's 2 x-measured rule).  Both errors are printed."""
    qkv, temperature, dout = _attn_inputs(1, 256, 257, 64, seed=3)
    ref = _attn_grads(_attn_ref, qkv, temperature, dout, torch.float64)
    t32 = _attn_grads(_attn_ref, qkv, temperature, dout, torch.float32)
    got = _attn_grads(_fused_attn, qkv, temperature, dout, torch.float32)
    e32, e = _errors(t32, ref, ATTN_GATES), _errors(got, ref, ATTN_GATES)
    _report("chan_attn long, float32 torch", e32)
    _report("chan_attn long, fused", e)
    for name, gate in ATTN_GATES.items():
        lim = max(gate, 2 * e32[name])
        assert e[name] < lim, f"{name}: error {e[name]:.3e} >= {lim:.3e} (project gate {gate:.0e}, float32 torch {e32[name]:.3e})"


def test_chan_attn_one_pixel():
    """A 1 x 1 image, C = 64, batch 2: every normalised channel is +-1; the forward is within the gate, all gradients are finite,
    dv and dtemperature within their gates, and dq, dk -- identically zero in the reference -- below 1e-6 in absolute value."""
    qkv, temperature, dout = _attn_inputs(2, 1, 1, 64, seed=11)
    ref = _attn_grads(_attn_ref, qkv, temperature, dout, torch.float64)
    got = _attn_grads(_fused_attn, qkv, temperature, dout, torch.float32)
    for name, t in got.items():
        assert bool(torch.isfinite(t).all()), name
    zq, zk = float(got["dq"].abs().max()), float(got["dk"].abs().max())
    print(f"[measured] chan_attn 1x1: max|dq|={zq:.2e} max|dk|={zk:.2e} (reference {float(ref['dq'].abs().max()):.1e} "
          f"{float(ref['dk'].abs().max()):.1e})")
    _assert_gates("chan_attn 1x1", got, ref, dict(out=OUT, dv=ACT, dtemperature=PARAM))
    assert zq < 1e-6 and zk < 1e-6, (zq, zk)


# ---- 5. dw conv + attention --------------------------------------------------------------------------------------------------------
CORE = ("qkv_pre", "dw_weight", "temperature")
CORE_GATES = dict(out=OUT, qkv_pre=ACT, dw_weight=PARAM, temperature=PARAM)


def _core_inputs(B, H, W, C, seed):
    """a qkv_pre whose CONVOLVED q and k are correlated: the k third is the permuted q third plus noise, and the depthwise taps
    of matched channels are equal"""
    qkv, temperature, dout = _attn_inputs(B, H, W, C, seed)
    g = torch.Generator().manual_seed(seed + 1)
    perm = torch.tensor([32 * (c // 32) + (5 * (c % 32) + 3) % 32 for c in range(C)])
    w = torch.randn(3 * C, 1, 3, 3, generator=g) / 3
    w[C:2 * C] = w[:C][perm]
    return dict(qkv_pre=qkv, dw_weight=w, temperature=temperature), dout


def _core_ref(a):
    C3 = a["qkv_pre"].shape[-1]
    qkv = F.conv2d(a["qkv_pre"].permute(0, 3, 1, 2), a["dw_weight"], None, padding=1, groups=C3).permute(0, 2, 3, 1)
    return _attn_ref(qkv, a["temperature"])


def _core_comp(a):
    """what a user has without tattn_core_fn, src/DADiff.py:266-281: NCHW conv, chunk, normalize, matmul, softmax, matmul"""
    x = a["qkv_pre"].permute(0, 3, 1, 2).contiguous()
    B, C3, H, W = x.shape
    heads = C3 // 96
    q, k, v = F.conv2d(x, a["dw_weight"], None, padding=1, groups=C3).chunk(3, dim=1)
    q, k, v = (t.reshape(B, heads, 32, H * W) for t in (q, k, v))
    q, k = F.normalize(q, dim=-1), F.normalize(k, dim=-1)
    attn = ((q @ k.transpose(-2, -1)) * a["temperature"].reshape(heads, 1, 1)).softmax(dim=-1)
    return (attn @ v).reshape(B, C3 // 3, H, W).permute(0, 2, 3, 1).contiguous()


def _core_fused(a):
    from founddiff_amd.tattn_train import tattn_core_fn
    return tattn_core_fn(a["qkv_pre"], a["dw_weight"], None, a["temperature"])


def _core_grads(fn, inputs, dout, dtype):
    a = {k: v.to("cuda", dtype).requires_grad_() for k, v in inputs.items()}
    out = fn(a)
    r = torch.autograd.grad(out, [a[k] for k in CORE], dout.to("cuda", dtype))
    return dict(out=out.detach(), **dict(zip(CORE, r)))


@pytest.mark.parametrize("C", [64, 256])
def test_core_against_float64(C):
    """tattn_core_fn (depthwise conv + attention) against F.conv2d + the reference formula in float64 on the GPU, 15 x 13,
    batch 2."""
    inputs, dout = _core_inputs(2, 15, 13, C, seed=C)
    ref = _core_grads(_core_ref, inputs, dout, torch.float64)
    got = _core_grads(_core_fused, inputs, dout, torch.float32)
    _assert_gates(f"core C={C}", got, ref, CORE_GATES)


def test_core_with_a_bias_against_float64():
    """the same with a qkv_dwconv bias (TransposedAttention(bias=True)), C = 64, 7 x 9"""
    from founddiff_amd.tattn_train import tattn_core_fn
    inputs, dout = _core_inputs(2, 7, 9, 64, seed=5)
    bias = 0.3 * torch.randn(192, generator=torch.Generator().manual_seed(6))
    res = {}
    for tag, dtype in (("ref", torch.float64), ("got", torch.float32)):
        a = {k: v.to("cuda", dtype).requires_grad_() for k, v in dict(inputs, dw_bias=bias).items()}
        if tag == "ref":
            qkv = F.conv2d(a["qkv_pre"].permute(0, 3, 1, 2), a["dw_weight"], a["dw_bias"], padding=1, groups=192).permute(0, 2, 3, 1)
            out = _attn_ref(qkv, a["temperature"])
        else:
            out = tattn_core_fn(a["qkv_pre"], a["dw_weight"], a["dw_bias"], a["temperature"])
        names = CORE + ("dw_bias",)
        res[tag] = dict(out=out.detach(), **dict(zip(names, torch.autograd.grad(out, [a[k] for k in names], dout.to("cuda", dtype)))))
    _assert_gates("core bias", res["got"], res["ref"], dict(CORE_GATES, dw_bias=PARAM))


# ---- 6. / 7. the modules against the reference's captures and float64 autograd through the oracle on the CPU -----------------------
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


def test_transposed_attention_module(golden):
    """tattn_train.TransposedAttention with the reference's weights (dim 64, 2 heads, 8 x 6): the output against the reference's
    capture, the gradients of x and of all four parameters against float64 autograd through oracle.nets.transposed_attention."""
    from founddiff_amd.tattn_train import TransposedAttention
    from oracle import nets
    g = golden("modules")
    sd = {k[len("tattn."):]: v for k, v in g.weights("tattn.").items()}
    m = TransposedAttention(64, 2)
    m.load_state_dict(sd, strict=True)
    _module_case("tattn", m.cuda(), sd, lambda s, x: nets.transposed_attention(nets.SD(s), x), dict(x=g["tattn.in"]), g["tattn.out"])


@pytest.mark.parametrize("file", ["modules", "modules_odd"])
def test_mamba_block_module(golden, file):
    """mamba_block_train.MambaBlock with the reference's mamba_c64 weights (4 x 6 and 5 x 5): the output against the capture,
    the gradients of x, c, t and all twenty parameters against float64 autograd through oracle.nets.mamba_block with
    selective_scan_torch."""
    from founddiff_amd.mamba_block_train import MambaBlock
    from oracle import nets
    g = golden(file)
    sd = {k[len("mamba_c64."):]: v for k, v in g.weights("mamba_c64.").items()}
    m = MambaBlock(64, 8, 128)
    m.load_state_dict(sd, strict=True)
    ref_fn = lambda s, x, c, t: nets.mamba_block(nets.SD(s), x, c, t, scan_fn=nets.selective_scan_torch)
    _module_case(f"mamba_block {file}", m.cuda(), sd, ref_fn, dict(x=g["mamba_c64.x"], c=g["mamba_c64.c"], t=g["mamba_c64.t"]),
                 g["mamba_c64.out"])


def test_mamba_block_rejects_hidden_32(golden):
    """mamba_c32 (hidden 32, 3C = 96): the documented RuntimeError"""
    from founddiff_amd.mamba_block_train import MambaBlock
    g = golden("modules")
    sd = {k[len("mamba_c32."):]: v for k, v in g.weights("mamba_c32.").items()}
    d_state = sd["mamba.A_logs"].shape[1]
    m = MambaBlock(32, d_state, 128)
    m.load_state_dict(sd, strict=True)
    with pytest.raises(RuntimeError, match="unsupported hidden_size=32"):
        m.cuda()(g["mamba_c32.x"].cuda(), g["mamba_c32.c"].cuda(), g["mamba_c32.t"].cuda())


# ---- 8. determinism and batch invariance ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def c128():
    inputs, dout = _core_inputs(2, 64, 64, 128, seed=21)
    return inputs, dout, _core_grads(_core_fused, inputs, dout, torch.float32)


def test_determinism(c128):
    """C = 128, 64 x 64, batch 2: a second forward + backward gives the same bits of out and every gradient"""
    inputs, dout, got = c128
    again = _core_grads(_core_fused, inputs, dout, torch.float32)
    for name in CORE_GATES:
        assert torch.equal(got[name], again[name]), name


def test_batch_invariance(c128):
    """slice 1 alone: the same bits of out and of qkv_pre's gradient as inside the batch of 2"""
    inputs, dout, got = c128
    alone = _core_grads(_core_fused, dict(inputs, qkv_pre=inputs["qkv_pre"][1:]), dout[1:], torch.float32)
    assert torch.equal(alone["out"], got["out"][1:])
    assert torch.equal(alone["qkv_pre"], got["qkv_pre"][1:])


# ---- 9. memory ---------------------------------------------------------------------------------------------------------------------
def test_memory_below_composition():
    """C = 64, 256 x 256, batch 2: the peak memory of one forward + backward of tattn_core_fn is below that of the torch
    composition (NCHW conv, chunk, normalize, matmul, softmax, matmul) in the same process."""
    inputs, dout = _core_inputs(2, 256, 256, 64, seed=31)
    a = {k: v.cuda().requires_grad_() for k, v in inputs.items()}
    dout = dout.cuda()

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = fn(a)
        g = torch.autograd.grad(out, [a[k] for k in CORE], dout)
        del out, g
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    fused = peak(_core_fused)
    comp = peak(_core_comp)
    print(f"[measured] peak memory: fused {fused / 2 ** 20:.0f} MB, composition {comp / 2 ** 20:.0f} MB")
    assert fused < comp, (fused, comp)


# ---- 10. binding ---------------------------------------------------------------------------------------------------------------------
class _AttnStandIn(torch.nn.Module):
    """the attributes TransposedAttention.forward reads (src/DADiff.py:252-260), built from torch layers alone"""

    def __init__(self, dim, heads):
        super().__init__()
        nn = torch.nn
        self.num_heads = heads
        self.temperature = nn.Parameter(torch.ones(heads, 1, 1))
        self.qkv = nn.Conv2d(dim, dim * 3, kernel_size=1, bias=False)
        self.qkv_dwconv = nn.Conv2d(dim * 3, dim * 3, kernel_size=3, stride=1, padding=1, groups=dim * 3, bias=False)
        self.project_out = nn.Conv2d(dim, dim, kernel_size=1, bias=False)


class _BlockStandIn(torch.nn.Module):
    """the attributes Mamba_block.forward reads (src/DADiff.py:457-474)"""

    def __init__(self, hidden_size, d_state, time_emb_dim):
        super().__init__()
        from founddiff_amd.ss2d_train import SS2D
        nn = torch.nn
        self.norm1 = nn.LayerNorm(hidden_size)
        self.mamba = SS2D(hidden_size, d_state)
        self.norm2 = nn.LayerNorm(hidden_size, elementwise_affine=False, eps=1e-6)
        self.adaLN_modulation = nn.Sequential(nn.SiLU(), nn.Linear(time_emb_dim, 6 * hidden_size, bias=True))
        self.cross = False
        self.attn_blk = _AttnStandIn(hidden_size, hidden_size // 32)


def test_binding():
    """A stand-in with the reference's attribute names and forward bound to mamba_block_forward gives the bits of MambaBlock with
    the same state dict (adaLN_modulation away from its zero initialisation, which gates both branches off); six Adam steps on a
    scalar loss lower it and every parameter gets a gradient; a half-precision module and input give a half-precision result and
    finite half-precision gradients.  The attention stand-in bound to transposed_attention_forward gives the bits of
    TransposedAttention."""
    from founddiff_amd import mamba_block_train as mbt, tattn_train as tat
    torch.manual_seed(9)
    m = mbt.MambaBlock(64, 8, 128)
    with torch.no_grad():
        for p in m.adaLN_modulation[-1].parameters():
            p.copy_(0.2 * torch.randn_like(p))
        m.attn_blk.temperature.add_(0.5 * torch.rand_like(m.attn_blk.temperature))
    m = m.cuda()
    s = _BlockStandIn(64, 8, 128).cuda()
    s.load_state_dict(m.state_dict(), strict=True)
    _BlockStandIn.forward = mbt.mamba_block_forward
    _AttnStandIn.forward = tat.transposed_attention_forward
    g = torch.Generator().manual_seed(10)
    x, c, t = (torch.randn(*shape, generator=g).cuda() for shape in ((2, 64, 12, 10), (2, 1, 256), (2, 128)))
    target = torch.randn(2, 64, 12, 10, generator=g).cuda()
    out = m(x, c, t)
    assert out.shape == x.shape and torch.equal(out, s(x, c, t))
    assert not torch.equal(out, x)                                  # the branches are open
    assert torch.equal(m.attn_blk(x), s.attn_blk(x))
    opt = torch.optim.Adam(s.parameters(), lr=1e-2)
    losses = []
    for _ in range(6):
        opt.zero_grad()
        loss = ((s(x, c, t) - target) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert all(p.grad is not None for p in s.parameters())
    assert losses[-1] < losses[0], losses
    h = mbt.MambaBlock(64, 8, 128)
    with torch.no_grad():
        for p in h.adaLN_modulation[-1].parameters():
            p.copy_(0.2 * torch.randn_like(p))
    h = h.cuda().half()
    xh = x.half().requires_grad_()
    out = h(xh, c.half(), t.half())
    assert out.dtype == torch.float16 and out.shape == x.shape
    out.float().sum().backward()
    assert xh.grad.dtype == torch.float16 and bool(torch.isfinite(xh.grad.float()).all())
    for name, p in h.named_parameters():
        assert p.grad is not None and p.grad.dtype == torch.float16 and bool(torch.isfinite(p.grad.float()).all()), name
