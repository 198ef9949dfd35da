"""founddiff_amd.adaln_train (csrc/fd_adaln_train.hip) and the Mamba_block built on it, against float64.

Gates, the project's own (tests/test_gpu_tattn_train.py), measured with conftest.rel_err (max abs error over the reference's max
abs value): < 1e-5 for forward outputs (and the per-pixel mean and rstd), < 1e-4 for dx, dy, dshift, dscale and dgate, < 1e-3 for
dgamma and dbeta.  torch's own fp32 composition stays below 1.0e-6 / 5.9e-7 / 7.4e-6 against float64 on these inputs (CPU, shapes
up to 512 x 512 x 64), so the gates leave at least 10 x room for a correct fp32 kernel.

Inputs: x = 8 rand per pixel + (0.5 + rand per pixel) randn per element -- every row carries an offset of up to 16 standard
deviations, so a variance that is not centred shows up; gamma = 1 + 0.3 randn; beta, shift, scale, gate = 0.3 .. 0.5 randn; y and
dout = randn.  Every test prints the errors it measured."""
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


def _assert_gates(tag, got, ref, gates):
    errs = {}
    for name in gates:
        assert got[name].shape == ref[name].shape, (name, got[name].shape, ref[name].shape)
        errs[name] = rel_err(got[name].cpu(), ref[name].cpu())
    _report(tag, errs)
    for name, gate in gates.items():
        assert errs[name] < gate, f"{tag}: {name} error {errs[name]:.3e} >= {gate:.0e}"


def _inputs(B, H, W, C, seed, affine=True):
    """fp32 on the GPU; mod is the (B, 6C) matrix whose column blocks 0, 1, 2 are shift, scale and gate"""
    g = torch.Generator().manual_seed(seed)
    rand, randn = (lambda *s: torch.rand(*s, generator=g)), (lambda *s: torch.randn(*s, generator=g))
    x = 8 * rand(B, H, W, 1) + (0.5 + rand(B, H, W, 1)) * randn(B, H, W, C)
    a = dict(x=x, gamma=1 + 0.3 * randn(C) if affine else None, beta=0.4 * randn(C) if affine else None,
             mod=torch.cat([0.5 * randn(B, C), 0.3 * randn(B, C), 0.4 * randn(B, C), randn(B, 3 * C)], dim=1),
             y=randn(B, H, W, C), dout=randn(B, H, W, C), dres=randn(B, H, W, C))
    return {k: (None if v is None else v.cuda()) for k, v in a.items()}


def _adaln_comp(x, gamma, beta, shift, scale, eps):
    """the torch composition the fused function replaces: F.layer_norm, then modulate"""
    n = F.layer_norm(x, x.shape[-1:], gamma, beta, eps)
    return n * (1 + scale[:, None, None, :]) + shift[:, None, None, :]


def _adaln_ref64(a, eps):
    """float64 autograd on the GPU: out, mean, rstd, dx, dshift, dscale, dgamma, dbeta"""
    C = a["x"].shape[-1]
    x = a["x"].double().requires_grad_()
    mod = a["mod"].double().requires_grad_()
    affine = a["gamma"] is not None
    gamma, beta = (a["gamma"].double().requires_grad_(), a["beta"].double().requires_grad_()) if affine else (None, None)
    out = _adaln_comp(x, gamma, beta, mod[:, :C], mod[:, C:2 * C], eps)
    r = torch.autograd.grad(out, [x, mod] + ([gamma, beta] if affine else []), a["dout"].double())
    ref = dict(out=out.detach(), dx=r[0], dshift=r[1][:, :C], dscale=r[1][:, C:2 * C],
               mean=x.detach().mean(-1), rstd=(x.detach().var(-1, unbiased=False) + eps).rsqrt())
    if affine:
        ref.update(dgamma=r[2], dbeta=r[3])
    return ref


def _adaln_gates(affine):
    gates = dict(out=OUT, mean=OUT, rstd=OUT, dx=ACT, dshift=ACT, dscale=ACT)
    return dict(gates, dgamma=PARAM, dbeta=PARAM) if affine else gates


HWS = [(1, 1), (3, 5), (1, 257), (130, 70)]


# ---- 1. adaLN through the C ABI -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("affine", [True, False], ids=["affine", "plain"])
@pytest.mark.parametrize("hw", HWS)
@pytest.mark.parametrize("C", [64, 128, 512])
def test_adaln_abi_against_float64(C, hw, affine):
    """fd_adaln_fwd_f32 / fd_adaln_bwd_f32, batch 2, eps 1e-5 with the affine and 1e-6 without: shift and scale read as columns
    of the (B, 6C) matrix (ld = 6C); dshift and dscale written into a sentinel-filled (B, 6C) matrix whose other columns must
    stay untouched; dout and x unchanged afterwards; dres NULL and dres = randn, dx against float64 in both cases."""
    from founddiff_amd import _lib as L
    H, W = hw
    B = 2
    eps = 1e-5 if affine else 1e-6
    a = _inputs(B, H, W, C, seed=C + H * W, affine=affine)
    x, dout, mod = a["x"], a["dout"], a["mod"]
    x0, dout0 = x.clone(), dout.clone()
    st = torch.cuda.current_stream().cuda_stream
    out, stats = torch.empty_like(x), torch.empty(B, H, W, 2, device="cuda")
    L.call("fd_adaln_fwd_f32", _ptr(x), _ptr(a["gamma"]), _ptr(a["beta"]), eps, _ptr(mod), _ptr(mod[:, C:]), 6 * C, _ptr(out),
           _ptr(stats), B, H * W, C, st)
    n = L.lib().fd_adaln_bwd_ws_floats(B, H * W, C)
    assert n > 0
    ws = torch.empty(n, device="cuda")
    ref = _adaln_ref64(a, eps)
    for dres in (None, a["dres"]):
        dx = torch.empty_like(x)
        dmod = torch.full((B, 6 * C), SENTINEL, device="cuda")
        dgamma, dbeta = (torch.empty(C, device="cuda"), torch.empty(C, device="cuda")) if affine else (None, None)
        L.call("fd_adaln_bwd_f32", _ptr(dout), _ptr(x), _ptr(stats), _ptr(a["gamma"]), _ptr(a["beta"]), _ptr(mod[:, C:]), 6 * C,
               _ptr(dres), _ptr(dx), _ptr(dmod), _ptr(dmod[:, C:]), 6 * C, _ptr(dgamma), _ptr(dbeta), _ptr(ws), B, H * W, C, st)
        torch.cuda.synchronize()
        assert bool((dmod[:, 2 * C:] == SENTINEL).all()), "columns beside dshift | dscale were written"
        assert torch.equal(x, x0) and torch.equal(dout, dout0), "x or dout was overwritten"
        got = dict(out=out, mean=stats[..., 0], rstd=stats[..., 1], dx=dx, dshift=dmod[:, :C], dscale=dmod[:, C:2 * C],
                   dgamma=dgamma, dbeta=dbeta)
        tag = f"adaln C={C} {H}x{W} affine={affine} dres={'set' if dres is not None else 'NULL'}"
        want = ref if dres is None else dict(ref, dx=ref["dx"] + dres.double())
        _assert_gates(tag, got, want, _adaln_gates(affine))


# ---- 2. the gated residual ------------------------------------------------------------------------------------------------------------
def _gate_grads(fn, a, dtype):
    C = a["x"].shape[-1]
    x, y, mod = (a[k].to(dtype).requires_grad_() for k in ("x", "y", "mod"))
    dout = a["dout"].to(dtype)
    out = fn(x, y, mod[:, 2 * C:3 * C])
    dx, dy, dmod = torch.autograd.grad(out, [x, y, mod], dout)
    return dict(out=out.detach(), dx=dx, dy=dy, dgate=dmod[:, 2 * C:3 * C]), dout


GATE_GATES = dict(out=OUT, dx=ACT, dy=ACT, dgate=ACT)


@pytest.mark.parametrize("hw", HWS)
@pytest.mark.parametrize("C", [64, 128, 512])
def test_gate_residual_against_float64(C, hw):
    """gate_residual_fn, batch 2, the gate read in place as columns [2C, 3C) of the (B, 6C) matrix; the gradient of x shares its
    storage with the incoming gradient: there is no copy"""
    from founddiff_amd.adaln_train import gate_residual_fn
    H, W = hw
    a = _inputs(2, H, W, C, seed=7 + C + H * W)
    ref, _ = _gate_grads(lambda x, y, g: x + g[:, None, None, :] * y, a, torch.float64)
    got, dout = _gate_grads(gate_residual_fn, a, torch.float32)
    assert got["dx"].data_ptr() == dout.data_ptr(), "the gradient of x is a copy"
    _assert_gates(f"gate_residual C={C} {H}x{W}", got, ref, GATE_GATES)


# ---- 3. the long reduction -----------------------------------------------------------------------------------------------------------
def _fn_grads(a, dtype, adaln, gate_res, eps=1e-5):
    """both functions on the same inputs: out, dx, dshift, dscale, dgamma, dbeta of adaLN; gout, gdx, dy, dgate of the gate"""
    C = a["x"].shape[-1]
    t = {k: a[k].to(dtype).requires_grad_() for k in ("x", "gamma", "beta", "mod", "y")}
    dout = a["dout"].to(dtype)
    mod = t["mod"]
    out = adaln(t["x"], t["gamma"], t["beta"], mod[:, :C], mod[:, C:2 * C], eps)
    dx, dgamma, dbeta, dmod = torch.autograd.grad(out, [t["x"], t["gamma"], t["beta"], mod], dout)
    gout = gate_res(t["x"], t["y"], mod[:, 2 * C:3 * C])
    gdx, dy, gmod = torch.autograd.grad(gout, [t["x"], t["y"], mod], dout)
    return dict(out=out.detach(), dx=dx, dshift=dmod[:, :C], dscale=dmod[:, C:2 * C], dgamma=dgamma, dbeta=dbeta,
                gout=gout.detach(), gdx=gdx, dy=dy, dgate=gmod[:, 2 * C:3 * C])


FN_GATES = dict(out=OUT, dx=ACT, dshift=ACT, dscale=ACT, dgamma=PARAM, dbeta=PARAM, gout=OUT, gdx=ACT, dy=ACT, dgate=ACT)


def _fused(a, **kw):
    from founddiff_amd.adaln_train import adaln_fn, gate_residual_fn
    return _fn_grads(a, torch.float32, adaln_fn, gate_residual_fn, **kw)


def _ref64(a, **kw):
    return _fn_grads(a, torch.float64, _adaln_comp, lambda x, y, g: x + g[:, None, None, :] * y, **kw)


def test_long_reduction():
    """B = 1, 512 x 512, C = 64: 262 144 pixels behind every entry of dshift, dscale, dgate, dgamma and dbeta (512 workgroup
    partials, two levels of sums), against float64 at the same gates"""
    a = _inputs(1, 512, 512, 64, seed=3)
    _assert_gates("long reduction", _fused(a), _ref64(a), FN_GATES)


# ---- 4. the autograd functions ----------------------------------------------------------------------------------------------------------
def test_functions_against_float64():
    """adaln_fn and gate_residual_fn at C = 128, 15 x 13, batch 2, every gradient"""
    a = _inputs(2, 15, 13, 128, seed=4)
    _assert_gates("functions", _fused(a), _ref64(a), FN_GATES)


def test_skip_gradient_joins_dx(monkeypatch):
    """adaln_skip_fn: a loss through both m and the skip; dx matches float64 autograd of LN-modulate(x) + x (weighted by two
    different gradients) at the activation gate, an unused skip gives the gradient of adaln_fn, and an unused m launches
    nothing: dx is the skip's gradient itself and the small gradients are zero"""
    from founddiff_amd import _lib as L
    from founddiff_amd.adaln_train import adaln_fn, adaln_skip_fn
    a = _inputs(2, 15, 13, 128, seed=5)
    C = 128
    res = {}
    for tag, dtype in (("ref", torch.float64), ("got", torch.float32)):
        x, gamma, beta, mod = (a[k].to(dtype).requires_grad_() for k in ("x", "gamma", "beta", "mod"))
        if tag == "ref":
            m, skip = _adaln_comp(x, gamma, beta, mod[:, :C], mod[:, C:2 * C], 1e-5), x
        else:
            m, skip = adaln_skip_fn(x, gamma, beta, mod[:, :C], mod[:, C:2 * C], 1e-5)
            assert skip.data_ptr() == x.data_ptr()
        loss = (m * a["dout"].to(dtype)).sum() + (skip * a["dres"].to(dtype)).sum()
        r = torch.autograd.grad(loss, [x, gamma, beta, mod])
        res[tag] = dict(dx=r[0], dgamma=r[1], dbeta=r[2], dshift=r[3][:, :C], dscale=r[3][:, C:2 * C])
    _assert_gates("skip", res["got"], res["ref"], dict(dx=ACT, dshift=ACT, dscale=ACT, dgamma=PARAM, dbeta=PARAM))
    x = a["x"].clone().requires_grad_()
    m, _ = adaln_skip_fn(x, a["gamma"], a["beta"], a["mod"][:, :C], a["mod"][:, C:2 * C], 1e-5)
    x2 = a["x"].clone().requires_grad_()
    m2 = adaln_fn(x2, a["gamma"], a["beta"], a["mod"][:, :C], a["mod"][:, C:2 * C], 1e-5)
    assert torch.equal(torch.autograd.grad(m, x, a["dout"])[0], torch.autograd.grad(m2, x2, a["dout"])[0])
    # only the skip used: dx is its gradient without a launch or a copy, the small gradients are zero
    x, gamma, mod = a["x"].clone().requires_grad_(), a["gamma"].clone().requires_grad_(), a["mod"].clone().requires_grad_()
    _, skip = adaln_skip_fn(x, gamma, a["beta"], mod[:, :C], mod[:, C:2 * C], 1e-5)
    calls, real = [], L.call
    monkeypatch.setattr(L, "call", lambda name, *args: (calls.append(name), real(name, *args))[1])
    dx, dgamma, dmod = torch.autograd.grad(skip, [x, gamma, mod], a["dres"])
    assert not calls and dx.data_ptr() == a["dres"].data_ptr()
    assert not bool(dgamma.any()) and not bool(dmod.any())


def test_bf16_inputs():
    """bf16 inputs give an fp32 result and finite bf16 gradients"""
    from founddiff_amd.adaln_train import adaln_fn, gate_residual_fn
    a = _inputs(2, 7, 9, 64, seed=6)
    C = 64
    t = {k: a[k].bfloat16().requires_grad_() for k in ("x", "gamma", "beta", "mod", "y")}
    mod = t["mod"]
    out = adaln_fn(t["x"], t["gamma"], t["beta"], mod[:, :C], mod[:, C:2 * C], 1e-5)
    out2 = gate_residual_fn(t["x"], t["y"], mod[:, 2 * C:3 * C])
    assert out.dtype == torch.float32 and out2.dtype == torch.float32
    e = rel_err(out.detach().cpu(), _adaln_comp(t["x"].float(), t["gamma"].float(), t["beta"].float(), mod[:, :C].float(),
                                       mod[:, C:2 * C].float(), 1e-5).detach().cpu())
    _report("bf16 inputs, out against the fp32 composition on the same values", dict(out=e))
    assert e < OUT
    leaves = [t[k] for k in ("x", "gamma", "beta", "mod", "y")]
    grads = torch.autograd.grad(out.sum() + (out2 * a["dout"]).sum(), leaves)
    for k, gr in zip(("x", "gamma", "beta", "mod", "y"), grads):
        assert gr.dtype == torch.bfloat16 and gr.shape == t[k].shape and bool(torch.isfinite(gr.float()).all()), k


# ---- 5. determinism and batch invariance -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def c128():
    a = _inputs(2, 64, 64, 128, seed=21)
    return a, _fused(a)


def test_determinism(c128):
    """C = 128, 64 x 64, batch 2: a second forward + backward gives the same bits of every output and gradient"""
    a, got = c128
    again = _fused(a)
    for name in FN_GATES:
        assert torch.equal(got[name], again[name]), name


def test_batch_invariance(c128):
    """slice 1 alone: the same bits of out, dx, dy, dshift, dscale and dgate as inside the batch of 2"""
    a, got = c128
    alone = _fused({k: (v if v.dim() == 1 else v[1:]) for k, v in a.items()})
    for name in ("out", "dx", "dshift", "dscale", "gout", "dy", "dgate"):
        assert torch.equal(alone[name], got[name][1:]), name


# ---- 6. memory -------------------------------------------------------------------------------------------------------------------------
def test_memory_below_composition():
    """C = 64, 256 x 256, batch 2: the peak memory of one forward + backward of adaln_fn is below that of the torch composition
    in the same process.  The composition keeps the LayerNorm output for the multiply by (1 + scale) beside x and passes
    full-size temporaries through both passes; the fused function keeps x and 2 floats per pixel."""
    from founddiff_amd.adaln_train import adaln_fn
    C = 64
    a = _inputs(2, 256, 256, C, seed=31)
    t = {k: a[k].requires_grad_() for k in ("x", "gamma", "beta", "mod")}

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = fn(t["x"], t["gamma"], t["beta"], t["mod"][:, :C], t["mod"][:, C:2 * C], 1e-5)
        g = torch.autograd.grad(out, list(t.values()), a["dout"])
        del out, g
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    fused = peak(adaln_fn)
    comp = peak(_adaln_comp)
    print(f"[measured] peak memory: fused {fused / 2 ** 20:.0f} MB, composition {comp / 2 ** 20:.0f} MB")
    assert fused < comp, (fused, comp)


# ---- 7. the block uses them -------------------------------------------------------------------------------------------------------------
def test_block_runs_on_the_fused_kernels(monkeypatch):
    """MambaBlock(64, 8, 128), adaLN_modulation moved off zero, 12 x 10, batch 2: the forward launches fd_adaln_fwd_f32 and
    fd_gate_res_fwd_f32 twice each, the backward each _bwd twice and every fd_adaln_bwd_f32 with a dres; the output and the
    gradients of x, c, t and all parameters match float64 autograd through oracle.nets.mamba_block on the CPU."""
    from founddiff_amd import _lib as L
    from founddiff_amd.mamba_block_train import MambaBlock
    from oracle import nets
    torch.manual_seed(9)
    m = MambaBlock(64, 8, 128)
    with torch.no_grad():
        for p in m.adaLN_modulation[-1].parameters():
            p.copy_(0.2 * torch.randn_like(p))
        m.norm1.weight.add_(0.3 * torch.randn_like(m.norm1.weight))
        m.norm1.bias.add_(0.3 * torch.randn_like(m.norm1.bias))
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    names = sorted(sd)
    g = torch.Generator().manual_seed(10)
    inputs = dict(x=torch.randn(2, 64, 12, 10, generator=g), c=torch.randn(2, 1, 256, generator=g), t=torch.randn(2, 128, generator=g))
    dout = torch.randn(2, 64, 12, 10, generator=g)
    sd64 = {k: v.double().requires_grad_() for k, v in sd.items()}
    in64 = {k: v.double().requires_grad_() for k, v in inputs.items()}
    o64 = nets.mamba_block(nets.SD(sd64), in64["x"], in64["c"], in64["t"], scan_fn=nets.selective_scan_torch)
    r = torch.autograd.grad(o64, list(in64.values()) + [sd64[k] for k in names], dout.double(), allow_unused=True)
    ref = dict(out=o64.detach(), **dict(zip(list(in64) + names, r)))

    calls, real = [], L.call

    def recording(name, *args):
        calls.append((name, args))
        return real(name, *args)
    monkeypatch.setattr(L, "call", recording)
    m = m.cuda()
    ing = {k: v.cuda().requires_grad_() for k, v in inputs.items()}
    o = m(**ing)
    fwd = [n for n, _ in calls]
    assert fwd.count("fd_adaln_fwd_f32") == 2 and fwd.count("fd_gate_res_fwd_f32") == 2, fwd
    assert not any(n.endswith("_bwd_f32") for n in fwd), fwd
    del calls[:]
    params = dict(m.named_parameters())
    assert sorted(params) == names
    r = torch.autograd.grad(o, list(ing.values()) + [params[k] for k in names], dout.cuda(), allow_unused=True)
    bwd = [n for n, _ in calls]
    assert bwd.count("fd_adaln_bwd_f32") == 2 and bwd.count("fd_gate_res_bwd_f32") == 2, bwd
    for n, args in calls:
        if n == "fd_adaln_bwd_f32":
            assert args[7] is not None and args[7].value, "fd_adaln_bwd_f32 was launched without a dres"
    got = dict(out=o.detach(), **dict(zip(list(ing) + names, r)))
    used = [k for k in ref if ref[k] is not None]
    assert all(got[k] is not None for k in used)
    _assert_gates("block", got, ref, dict(out=OUT, **{k: (ACT if k in inputs else PARAM) for k in used if k != "out"}))
