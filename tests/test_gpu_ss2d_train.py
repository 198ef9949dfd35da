"""founddiff_amd.ss2d_train (csrc/fd_ss2d_train.hip, the NHWC entries of csrc/fd_cross_scan_bwd.hip) against float64 and against
the reference's captured outputs.

Gates against float64, rel_err = max abs error over the reference's max abs value: < 1e-5 for forward outputs, < 1e-4 for
gradients of activations, < 1e-3 for parameter gradients (sums over batch x pixels).  The SS2D core is held to CORE_GATES, the
gates of test_gpu_scan_bwd.py and test_gpu_cross_scan_train.py: 1e-5 and 1e-4.  Against the reference's captured fp32 outputs:
< 1e-4, as test_gpu_e2e.py::test_mamba_block[fp32].  Measured errors are in each test's docstring."""
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
from test_gpu_cross_scan_train import BLOCK_SHAPES, _ScanF64, _params, _ref_y

pytestmark = pytest.mark.gpu

ACT, PARAM, OUT = 1e-4, 1e-3, 1e-5
CORE = ("xz", "conv_weight", "conv_bias", "x_proj_weight", "dt_projs_weight", "dt_projs_bias", "A_logs", "Ds", "norm_weight",
        "norm_bias", "local")
# the core: 1e-5 for out and the activation gradients, 1e-4 for the parameter gradients, as test_gpu_scan_bwd_cases.py holds the scan
# backward underneath (measured on an MI355X: activations up to 4.5e-7, parameters up to 2.2e-6)
CORE_GATES = dict(out=OUT, xz=1e-5, local=1e-5, **{k: 1e-4 for k in CORE[1:-1]})
SENTINEL = -12345.0


def _ptr(t):
    return None if t is None else t.data_ptr()


def _report(tag, errs):
    print(f"[measured] {tag}: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))


def _assert_gates(tag, got, ref, gates):
    errs = {}
    for name, gate in gates.items():
        assert got[name].shape == ref[name].shape, (tag, name, got[name].shape, ref[name].shape)
        errs[name] = rel_err(got[name].cpu(), ref[name].cpu())
    _report(tag, errs)
    for name, gate in gates.items():
        assert errs[name] < gate, f"{tag}: {name} error {errs[name]:.3e} >= {gate:.0e}"


# ---- 1a. SiLU(dwconv3x3 + bias) backward ------------------------------------------------------------------------------------
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("hw", [(3, 5), (15, 13), (64, 64), (130, 70)])
@pytest.mark.parametrize("C", [64, 128, 1024])
def test_dwconv_silu_backward(C, hw, bias):
    """fd_dwconv3x3_silu_bwd_f32 against float64 autograd through F.conv2d + F.silu on the GPU, batch 2: x read in place from
    the first half of a (B, H, W, 2C) tensor, dx written into the first half of a sentinel-filled one whose second half must stay
    untouched.  Measured on an MI355X: dx 0.7e-7 .. 2.1e-7, dweight 0.8e-7 .. 2.4e-7, dbias 0.8e-7 .. 2.6e-7."""
    from founddiff_amd import _lib as L
    H, W = hw
    B = 2
    g = torch.Generator().manual_seed(C + H * W)
    xz = torch.randn(B, H, W, 2 * C, generator=g)
    w = torch.randn(C, 1, 3, 3, generator=g) / 3
    b = 0.1 * torch.randn(C, generator=g) if bias else None
    dout = torch.randn(B, H, W, C, generator=g)
    # float64
    x64 = xz[..., :C].cuda().double().requires_grad_()
    w64 = w.cuda().double().requires_grad_()
    b64 = b.cuda().double().requires_grad_() if bias else None
    y = F.silu(F.conv2d(x64.permute(0, 3, 1, 2), w64, b64, padding=1, groups=C)).permute(0, 2, 3, 1)
    ref = torch.autograd.grad(y, [x64, w64] + ([b64] if bias else []), dout.cuda().double())
    # the kernel
    xzd, w9 = xz.cuda(), w.reshape(C, 9).t().contiguous().cuda()
    bd = b.cuda() if bias else None
    dpre = dout.cuda().clone()
    dxz = torch.full((B, H, W, 2 * C), SENTINEL, device="cuda")
    dw9, db = torch.empty(9, C, device="cuda"), (torch.empty(C, device="cuda") if bias else None)
    n = L.lib().fd_dwconv3x3_silu_bwd_ws_floats(B, H, W, C)
    assert n > 0
    ws = torch.empty(n, device="cuda")
    L.call("fd_dwconv3x3_silu_bwd_f32", _ptr(xzd), 2 * C, 0, _ptr(w9), _ptr(bd), _ptr(dpre), _ptr(dxz), 2 * C, 0, _ptr(dw9), _ptr(db),
           _ptr(ws), B, H, W, C, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert bool((dxz[..., C:] == SENTINEL).all()), "the other half of dxz was written"
    got = dict(dx=dxz[..., :C], dweight=dw9.t().reshape(C, 1, 3, 3))
    want = dict(dx=ref[0], dweight=ref[1])
    gates = dict(dx=ACT, dweight=PARAM)
    if bias:
        got["dbias"], want["dbias"], gates["dbias"] = db, ref[2], PARAM
    _assert_gates(f"dwconv_silu_bwd C={C} {H}x{W} bias={bias}", got, want, gates)


# ---- 1b. LN * SiLU(z) + local, forward and backward ----------------------------------------------------------------------------
@pytest.mark.parametrize("local", [True, False], ids=["local", "nolocal"])
@pytest.mark.parametrize("hw", [1, 63, 4099])
@pytest.mark.parametrize("C", [64, 128, 1024])
def test_ln_silu_gate(C, hw, local):
    """fd_ln_silu_gate_fwd_f32 / _bwd_f32 against float64 autograd through F.layer_norm, F.silu on the GPU, batch 3: z read in
    place from the second half of a (B, hw, 2C) tensor, dz written into the second half of a sentinel-filled one.  Measured on an
    MI355X: out 0.8e-7 .. 1.6e-7, dy 0.9e-7 .. 2.3e-7, dz 1.0e-7 .. 1.8e-7, dgamma / dbeta 0.5e-7 .. 2.3e-7, dlocal 0 (one
    pixel: a copy) .. 2.1e-7."""
    from founddiff_amd import _lib as L
    B = 3
    g = torch.Generator().manual_seed(C + hw)
    y = torch.randn(B, hw, C, generator=g) * 2 + 0.5
    xz = torch.randn(B, hw, 2 * C, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    loc = torch.randn(B, C, generator=g) if local else None
    dout = torch.randn(B, hw, C, generator=g)
    # float64
    leaves = [t.cuda().double().requires_grad_() for t in (y, xz[..., C:], gamma, beta)]
    o = F.layer_norm(leaves[0], (C,), leaves[2], leaves[3], 1e-5) * F.silu(leaves[1])
    if local:
        leaves.append(loc.cuda().double().requires_grad_())
        o = o + leaves[4][:, None]
    ref = torch.autograd.grad(o, leaves, dout.cuda().double())
    # the kernels
    yd, xzd, gd, bd, dd = y.cuda(), xz.cuda(), gamma.cuda(), beta.cuda(), dout.cuda()
    ld = loc.cuda() if local else None
    out, stats = torch.empty(B, hw, C, device="cuda"), torch.empty(B, hw, 2, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    L.call("fd_ln_silu_gate_fwd_f32", _ptr(yd), _ptr(gd), _ptr(bd), 1e-5, _ptr(xzd), 2 * C, C, _ptr(ld), C, _ptr(out), _ptr(stats),
           B, hw, C, s)
    dy = torch.empty(B, hw, C, device="cuda")
    dxz = torch.full((B, hw, 2 * C), SENTINEL, device="cuda")
    dg, db = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    dl = torch.empty(B, C, device="cuda") if local else None
    n = L.lib().fd_ln_silu_gate_bwd_ws_floats(B, hw, C)
    assert n > 0
    ws = torch.empty(n, device="cuda")
    L.call("fd_ln_silu_gate_bwd_f32", _ptr(dd), _ptr(yd), _ptr(stats), _ptr(gd), _ptr(bd), _ptr(xzd), 2 * C, C, _ptr(dy), _ptr(dxz),
           2 * C, C, _ptr(dg), _ptr(db), _ptr(dl), _ptr(ws), B, hw, C, s)
    torch.cuda.synchronize()
    assert bool((dxz[..., :C] == SENTINEL).all()), "the other half of dxz was written"
    got = dict(out=out, dy=dy, dz=dxz[..., C:], dgamma=dg, dbeta=db)
    want = dict(out=o.detach(), dy=ref[0], dz=ref[1], dgamma=ref[2], dbeta=ref[3])
    gates = dict(out=OUT, dy=ACT, dz=ACT, dgamma=PARAM, dbeta=PARAM)
    if local:
        got["dlocal"], want["dlocal"], gates["dlocal"] = dl, ref[4], ACT
    _assert_gates(f"ln_silu_gate C={C} hw={hw} local={local}", got, want, gates)


# ---- 2. / 3. the module against the reference's captures and against float64 autograd on the CPU ---------------------------------
TAGS = {"c32n4": (32, 4), "c64n32": (64, 32), "c32n16": (32, 16)}


def _golden_module(golden, file, tag):
    from founddiff_amd.ss2d_train import SS2D
    g = golden(file)
    prefix = f"ss2d_{tag}."
    sd = {k[len(prefix):]: v for k, v in g.weights(prefix).items()}
    m = SS2D(*TAGS[tag])
    m.load_state_dict(sd, strict=True)
    return m.cuda(), sd, g[prefix + "x"], g[prefix + "c"], g[prefix + "out"]


@pytest.mark.parametrize("file", ["modules", "modules_odd"])
@pytest.mark.parametrize("tag", sorted(TAGS))
def test_module_forward_against_the_reference(golden, file, tag):
    """SS2D with the reference's weights against the reference's captured output (even and odd H / W).  Measured on an MI355X:
    2.2e-7 .. 4.1e-7."""
    m, _, x, c, out = _golden_module(golden, file, tag)
    with torch.no_grad():
        got = m(x.cuda(), c.cuda())
    e = rel_err(got.cpu(), out)
    _report(f"module forward {file} {tag}", dict(out=e))
    assert got.shape == out.shape and e < 1e-4, e


def _module_grads_case(m, sd, x, c, tag):
    from oracle import nets
    g = torch.Generator().manual_seed(5)
    dout = torch.randn(x.shape[:3] + (sd["out_proj.weight"].shape[0],), generator=g)
    # float64 autograd on the CPU through the oracle
    sd64 = {k: v.double().requires_grad_() for k, v in sd.items()}
    x64, c64 = x.double().requires_grad_(), c.double().requires_grad_()
    o64 = nets.ss2d(sd64, x64, c64, scan_fn=nets.selective_scan_torch)
    names = sorted(sd)
    r = torch.autograd.grad(o64, [x64, c64] + [sd64[k] for k in names], dout.double())
    ref = dict(out=o64.detach(), x=r[0], c=r[1], **dict(zip(names, r[2:])))
    xg, cg = x.cuda().requires_grad_(), c.cuda().requires_grad_()
    o = m(xg, cg)
    params = dict(m.named_parameters())
    assert sorted(params) == names
    r = torch.autograd.grad(o, [xg, cg] + [params[k] for k in names], dout.cuda())
    got = dict(out=o.detach(), x=r[0], c=r[1], **dict(zip(names, r[2:])))
    _assert_gates(f"module grads {tag}", got, ref, dict(out=OUT, x=ACT, c=ACT, **{k: PARAM for k in names}))


@pytest.mark.parametrize("file", ["modules", "modules_odd"])
@pytest.mark.parametrize("tag", sorted(TAGS))
def test_module_gradients_at_the_golden_shapes(golden, file, tag):
    """x, c and all twelve parameters against float64 autograd on the CPU through oracle.nets.ss2d with selective_scan_torch.
    Measured on an MI355X: out 1.8e-7 .. 4.7e-7, x / c 2.4e-7 .. 7.5e-7, parameters 1.1e-7 .. 8.0e-7."""
    m, sd, x, c, _ = _golden_module(golden, file, tag)
    _module_grads_case(m, sd, x, c, f"{file} {tag}")


@pytest.mark.parametrize("case", [(64, 4, 16, 16), (128, 16, 15, 13)])
def test_module_gradients_at_block_widths(case):
    """The same at d_model 64 / N 4 / 16 x 16 and d_model 128 / N 16 / 15 x 13 (d_inner 128 and 256), the module's own
    initialisation, batch 2.  Measured on an MI355X: out 4.2e-7 .. 1.1e-6, x / c 3.1e-7 .. 8.4e-7, parameters 2.0e-7 .. 1.7e-6."""
    from founddiff_amd.ss2d_train import SS2D
    d_model, N, H, W = case
    torch.manual_seed(d_model + N)
    m = SS2D(d_model, N)
    with torch.no_grad():         # away from the symmetric points of the default initialisation (out_norm 1 / 0, Ds 1)
        for k, p in m.named_parameters():
            if k.startswith("out_norm") or k in ("Ds", "A_logs", "conv2d.bias"):
                p.add_(0.1 * torch.randn_like(p))
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(6)
    x, c = torch.randn(2, H, W, d_model, generator=g), torch.randn(2, 1, 256, generator=g)
    _module_grads_case(m.cuda(), sd, x, c, f"{case}")


# ---- 4. / 5. the core function against a float64 composition on the GPU -------------------------------------------------------------
def _core_inputs(B, H, W, D, N, R, seed):
    g = torch.Generator().manual_seed(seed)
    p = _params(D, N, R, seed=seed + 1)
    return dict(xz=torch.randn(B, H, W, 2 * D, generator=g), conv_weight=torch.randn(D, 1, 3, 3, generator=g) / 3,
                conv_bias=0.1 * torch.randn(D, generator=g), **p, norm_weight=1 + 0.1 * torch.randn(D, generator=g),
                norm_bias=0.1 * torch.randn(D, generator=g), local=torch.randn(B, D, generator=g)), \
        torch.randn(B, H, W, D, generator=g)


def _core_f64(a):
    D = a["norm_weight"].shape[0]
    x, z = a["xz"].chunk(2, dim=-1)
    xi = F.silu(F.conv2d(x.permute(0, 3, 1, 2), a["conv_weight"], a["conv_bias"], padding=1, groups=D))
    y = _ref_y(xi, a, _ScanF64.apply)
    return F.layer_norm(y, (D,), a["norm_weight"], a["norm_bias"], 1e-5) * F.silu(z) + a["local"][:, None, None, :]


def _core_fused(a):
    from founddiff_amd.ss2d_train import ss2d_core_fn
    return ss2d_core_fn(*[a[k] for k in CORE])


def _core_grads(fn, inputs, dout, dtype):
    a = {k: v.to("cuda", dtype).requires_grad_() for k, v in inputs.items()}
    out = fn(a)
    r = torch.autograd.grad(out, [a[k] for k in CORE], dout.to("cuda", dtype))
    return dict(out=out.detach(), **dict(zip(CORE, r)))


@pytest.mark.parametrize("shape", BLOCK_SHAPES)
def test_core_at_every_block_shape(shape):
    """ss2d_core_fn at every (d_inner, N, R) of the architecture, 64 x 64, batch 2, against torch conv / LayerNorm / SiLU in
    float64 around the float64 scan reference.  Measured on an MI355X: out 1.5e-7 .. 4.5e-7, dxz 2.0e-7 .. 3.7e-7, dlocal
    1.2e-7 .. 1.8e-7, parameter gradients 1.4e-7 .. 1.5e-6."""
    D, N, R = shape
    inputs, dout = _core_inputs(2, 64, 64, D, N, R, seed=D + N + R)
    ref = _core_grads(_core_f64, inputs, dout, torch.float64)
    got = _core_grads(_core_fused, inputs, dout, torch.float32)
    _assert_gates(f"core {shape}", got, ref, CORE_GATES)


@pytest.fixture(scope="module")
def level0():
    """down0 at the training size (train.py: batch 2 at 512 x 512): d_inner 128, N 4, R 4"""
    inputs, dout = _core_inputs(2, 512, 512, 128, 4, 4, seed=41)
    got = _core_grads(_core_fused, inputs, dout, torch.float32)
    ref = {k: v.float() for k, v in _core_grads(_core_f64, inputs, dout, torch.float64).items()}
    torch.cuda.empty_cache()
    return inputs, dout, got, ref


def test_level0_training_size(level0):
    """Level 0 against float64.  Measured on an MI355X: out 2.6e-7, dxz 3.0e-7, dlocal 2.5e-7, parameter gradients 2.1e-7 ..
    2.2e-6 (A_logs: sums over 2 x 65536 positions per direction)."""
    _, _, got, ref = level0
    _assert_gates("core level 0", got, ref, CORE_GATES)


def test_determinism_level0(level0):
    """A second forward + backward on the same inputs: the same bits in out and all eleven gradients."""
    inputs, dout, got, _ = level0
    again = _core_grads(_core_fused, inputs, dout, torch.float32)
    for name in CORE_GATES:
        assert torch.equal(got[name], again[name]), name


def test_batch_invariance_level0(level0):
    """Slice 1 of the level-0 batch alone: the same bits of out and dxz as inside the batch of 2."""
    inputs, dout, got, _ = level0
    one = {k: (v[1:] if k in ("xz", "local") else v) for k, v in inputs.items()}
    alone = _core_grads(_core_fused, one, dout[1:], torch.float32)
    assert torch.equal(alone["out"], got["out"][1:])
    assert torch.equal(alone["xz"], got["xz"][1:])
    assert torch.equal(alone["local"], got["local"][1:])


# ---- 6. memory ---------------------------------------------------------------------------------------------------------------------
def _comp(a):
    """what a user has without ss2d_core_fn: SS2D.forward's torch glue around cross_scan_train.cross_selective_scan"""
    from founddiff_amd.cross_scan_train import cross_selective_scan
    D = a["norm_weight"].shape[0]
    x, z = a["xz"].chunk(2, dim=-1)
    z = F.silu(z)
    x = x.permute(0, 3, 1, 2).contiguous()
    x = F.silu(F.conv2d(x, a["conv_weight"], a["conv_bias"], padding=1, groups=D))
    norm = lambda y: F.layer_norm(y, (D,), a["norm_weight"], a["norm_bias"], 1e-5)
    y = cross_selective_scan(x, a["x_proj_weight"], None, a["dt_projs_weight"], a["dt_projs_bias"], a["A_logs"], a["Ds"], norm,
                             nrows=1, delta_softplus=True, step_size=2)
    return y * z + a["local"][:, None, None, :]


def test_memory_below_composition_at_down0():
    """down0, batch 2: the peak memory of one forward + backward of ss2d_core_fn is below that of the torch glue around
    cross_scan_train.cross_selective_scan in the same process.  Measured on an MI355X (tools/ss2d_train_bench.py): 1880 MB
    against 2432 MB."""
    inputs, dout = _core_inputs(2, 512, 512, 128, 4, 4, seed=51)
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
    comp = peak(_comp)
    print(f"[measured] peak memory: fused {fused / 2 ** 20:.0f} MB, composition {comp / 2 ** 20:.0f} MB")
    assert fused < comp, (fused, comp)


# ---- 7. binding ------------------------------------------------------------------------------------------------------------------
class _StandIn(torch.nn.Module):
    """the attributes SS2D.forward reads (src/emamba2.py:404-532), built from torch layers alone"""

    def __init__(self, d_model, d_state):
        super().__init__()
        nn = torch.nn
        D, R = 2 * d_model, math.ceil(d_model / 16)
        self.d_conv, self.step_size, self.ssm_low_rank = 3, 2, False
        self.in_proj = nn.Linear(d_model, 2 * D, bias=False)
        self.conv2d = nn.Conv2d(D, D, 3, padding=1, groups=D, bias=True)
        self.x_proj_weight = nn.Parameter(torch.zeros(4, R + 2 * d_state, D))
        self.dt_projs_weight = nn.Parameter(torch.zeros(4, D, R))
        self.dt_projs_bias = nn.Parameter(torch.zeros(4, D))
        self.A_logs = nn.Parameter(torch.zeros(4 * D, d_state))
        self.Ds = nn.Parameter(torch.zeros(4 * D))
        self.out_norm = nn.LayerNorm(D)
        self.out_proj = nn.Linear(D, d_model, bias=False)
        self.dropout = nn.Identity()
        self.attn = nn.Sequential(nn.Linear(256, D, bias=False), nn.SiLU())


def test_binding():
    """A stand-in with the reference's attribute names and forward bound to ss2d_forward gives the bits of ss2d_train.SS2D with
    the same state dict; six Adam steps on a scalar loss lower it; a half-precision module and x give a half-precision result
    and gradient."""
    from founddiff_amd import ss2d_train as sst
    torch.manual_seed(9)
    m = sst.SS2D(32, 4).cuda()
    s = _StandIn(32, 4).cuda()
    s.load_state_dict(m.state_dict(), strict=True)
    _StandIn.forward = sst.ss2d_forward
    g = torch.Generator().manual_seed(10)
    x, c = torch.randn(2, 12, 10, 32, generator=g).cuda(), torch.randn(2, 1, 256, generator=g).cuda()
    target = torch.randn(2, 12, 10, 32, generator=g).cuda()
    assert torch.equal(m(x, c), s(x, c))
    opt = torch.optim.Adam(s.parameters(), lr=1e-2)
    losses = []
    for _ in range(6):
        opt.zero_grad()
        loss = ((s(x, c) - target) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert all(p.grad is not None for p in s.parameters())
    assert losses[-1] < losses[0], losses
    h = sst.SS2D(32, 4).cuda().half()
    xh = x.half().requires_grad_()
    out = h(xh, c.half())
    assert out.dtype == torch.float16 and out.shape == x.shape
    out.float().sum().backward()
    assert xh.grad.dtype == torch.float16 and h.A_logs.grad.dtype == torch.float16
    assert bool(torch.isfinite(xh.grad.float()).all())
