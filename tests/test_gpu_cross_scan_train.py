"""founddiff_amd.cross_scan_train (include/founddiff_hip.h: fd_cross_scan_fwd_f32 / fd_cross_scan_bwd_f32,
csrc/fd_cross_scan_bwd.hip) against float64: autograd on the CPU through the oracle's cross_selective_scan with
selective_scan_torch for small images, and on the GPU through the oracle's efficient_scan / efficient_merge, the two einsums and a
test-local autograd wrapper around tests/scan_bwd_ref.py for the block shapes and level 0.

Gates (those of test_gpu_scan_bwd.py): rel_err < 1e-5 for y and dx, < 1e-4 for the weight gradients (sums over
batch x L); rel_err = max abs error over the reference's max abs value.  Every comparison prints its error
before it asserts (pytest -s); the docstrings quote the figures of one run on an MI355X."""
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
from scan_bwd_cases import _params, _ref_y, _ScanF64, _x          # noqa: F401 (test_gpu_ss2d_train.py imports them from here)

pytestmark = pytest.mark.gpu

BLOCK_SHAPES = [(128, 4, 4), (128, 8, 4), (256, 16, 8), (512, 32, 16), (1024, 32, 32), (512, 16, 16), (256, 8, 8)]  # (d_inner, N, R)
PARAMS = ("x_proj_weight", "dt_projs_weight", "dt_projs_bias", "A_logs", "Ds")
GATES = dict(y=1e-5, x=1e-5, x_proj_weight=1e-4, dt_projs_weight=1e-4, dt_projs_bias=1e-4, A_logs=1e-4, Ds=1e-4)


def _grads(fn, x, p, dy, device, dtype):
    xx = x.to(device, dtype).requires_grad_()
    pp = {k: v.to(device, dtype).requires_grad_() for k, v in p.items()}
    y = fn(xx, pp)
    g = torch.autograd.grad(y, [xx] + [pp[k] for k in PARAMS], dy.to(device, dtype))
    return dict(y=y.detach(), x=g[0], **dict(zip(PARAMS, g[1:])))


def _fused(x, p):
    from founddiff_amd.cross_scan_train import cross_scan_fn
    return cross_scan_fn(x, *[p[k] for k in PARAMS])


def _check(got, ref, tag):
    for name, gate in GATES.items():
        assert got[name].shape == ref[name].shape, (tag, name)
        e = rel_err(got[name].cpu(), ref[name].cpu())
        print(f"cross_scan_train[{tag}] {name} {e:.3e}")
        assert e < gate, f"{tag}: {name} error {e:.3e} >= {gate:.0e}"


@pytest.mark.parametrize("shape", [(128, 4, 4), (256, 16, 8)])
@pytest.mark.parametrize("hw", [(16, 16), (15, 13)])
def test_small_against_cpu_autograd(shape, hw):
    """The public function with a LayerNorm out_norm against float64 autograd on the CPU through
    oracle.nets.cross_selective_scan(sd, x, scan_fn=nets.selective_scan_torch), batch 2; 15 x 13 is the odd-size padding check.
    Measured on an MI355X: y 3.8e-7 .. 7.6e-7, dx 3.9e-7 .. 7.0e-7, weight gradients 1.0e-7 .. 9.2e-7."""
    from founddiff_amd.cross_scan_train import cross_selective_scan
    from oracle import nets
    D, N, R = shape
    H, W = hw
    p = _params(D, N, R, seed=D + N + H)
    p["out_norm.weight"] = 1 + 0.1 * torch.randn(D, generator=torch.Generator().manual_seed(3))
    p["out_norm.bias"] = 0.1 * torch.randn(D, generator=torch.Generator().manual_seed(4))
    x, dy = _x(2, D, H, W, seed=H * W + D)

    def ref_fn(xx, pp):
        return nets.cross_selective_scan(pp, xx, scan_fn=nets.selective_scan_torch)

    def got_fn(xx, pp):
        norm = torch.nn.LayerNorm(D, eps=1e-5).cuda()
        with torch.no_grad():
            norm.weight.copy_(pp["out_norm.weight"])
            norm.bias.copy_(pp["out_norm.bias"])
        return cross_selective_scan(xx, pp["x_proj_weight"], None, pp["dt_projs_weight"], pp["dt_projs_bias"], pp["A_logs"],
                                    pp["Ds"], norm, nrows=1, delta_softplus=True, step_size=2)

    ref = _grads(ref_fn, x, p, dy, "cpu", torch.float64)
    got = _grads(got_fn, x, p, dy, "cuda", torch.float32)
    _check(got, ref, f"{shape} {hw}")


@pytest.mark.parametrize("shape", BLOCK_SHAPES)
def test_every_block_shape(shape):
    """Every (d_inner, N, R) of the architecture at 64 x 64 (L = 1024 per direction), batch 2, against the float64 GPU
    reference.  Measured on an MI355X: y 4.3e-7 .. 1.5e-6, dx 4.4e-7 .. 1.3e-6, weight gradients 0.9e-7 .. 1.3e-6."""
    D, N, R = shape
    p = _params(D, N, R, seed=D + N + R)
    x, dy = _x(2, D, 64, 64, seed=D * N)
    ref = _grads(lambda xx, pp: _ref_y(xx, pp, _ScanF64.apply), x, p, dy, "cuda", torch.float64)
    got = _grads(_fused, x, p, dy, "cuda", torch.float32)
    _check(got, ref, f"{shape}")


@pytest.fixture(scope="module")
def level0():
    """down0 at the training size (train.py: batch 2 at 512 x 512): d_inner 128, N 4, R 4, L = 65536 per direction"""
    p = _params(128, 4, 4, seed=17)
    x, dy = _x(2, 128, 512, 512, seed=18)
    got = _grads(_fused, x, p, dy, "cuda", torch.float32)
    ref = _grads(lambda xx, pp: _ref_y(xx, pp, _ScanF64.apply), x, p, dy, "cuda", torch.float64)
    ref = {k: v.float() for k, v in ref.items()}
    torch.cuda.empty_cache()
    return p, x, dy, got, ref


def test_level0_training_size(level0):
    """Level 0 against float64 (256 tiles of carries per row).  Measured on an MI355X: y 5.3e-7, dx 6.8e-7, weight gradients
    4.1e-7 .. 3.4e-6 (A_logs: sums over 2 x 65536 positions)."""
    p, x, dy, got, ref = level0
    _check(got, ref, "level 0")


def test_determinism_level0(level0):
    """A second forward + backward on the same inputs gives the same bits in y and all six gradients (no float atomics)."""
    p, x, dy, got, _ = level0
    again = _grads(_fused, x, p, dy, "cuda", torch.float32)
    for name in GATES:
        assert torch.equal(got[name], again[name]), name


def test_batch_invariance(level0):
    """Slice 1 of the level-0 batch alone: the same bits of y and dx as inside the batch of 2."""
    p, x, dy, got, _ = level0
    one = _grads(_fused, x[1:], p, dy[1:], "cuda", torch.float32)
    assert torch.equal(one["y"], got["y"][1:])
    assert torch.equal(one["x"], got["x"][1:])


def test_reference_call_pattern():
    """forward_corev2's argument list (src/emamba2.py:704-708) in an SS2D-shaped graph -- dwconv + SiLU in front, the gate and
    out_proj behind, a scalar loss -- against the same graph in float64 on the CPU through the oracle; then a few Adam steps on
    the GPU lower the loss.  Also: a 16-bit input comes back in its dtype, a wrong shape raises."""
    from founddiff_amd.cross_scan_train import cross_selective_scan
    from oracle import nets
    B, C, H, W, N, R = 2, 32, 12, 10, 4, 4
    D = 2 * C
    g = torch.Generator().manual_seed(21)
    p = _params(D, N, R, seed=22)
    p.update(conv_w=torch.randn(D, 1, 3, 3, generator=g) / 3, out_w=torch.randn(C, D, generator=g) * D ** -0.5)
    x0 = torch.randn(B, D, H, W, generator=g)
    z = torch.randn(B, H, W, D, generator=g)
    target = torch.randn(B, H, W, C, generator=g)

    def loss_of(pp, dev, dtype, fused):
        xi = F.silu(F.conv2d(x0.to(dev, dtype), pp["conv_w"], padding=1, groups=D))
        norm = torch.nn.LayerNorm(D).to(dev, dtype)
        if fused:
            y = cross_selective_scan(xi, pp["x_proj_weight"], None, pp["dt_projs_weight"], pp["dt_projs_bias"], pp["A_logs"],
                                     pp["Ds"], norm, nrows=1, delta_softplus=True, step_size=2)
        else:
            sd = dict(pp, **{"out_norm.weight": norm.weight, "out_norm.bias": norm.bias})
            y = nets.cross_selective_scan(sd, xi, scan_fn=nets.selective_scan_torch)
        out = F.linear(y * z.to(dev, dtype), pp["out_w"])
        return ((out - target.to(dev, dtype)) ** 2).mean()

    pr = {k: v.double().requires_grad_() for k, v in p.items()}
    l_ref = loss_of(pr, "cpu", torch.float64, False)
    l_ref.backward()
    pg = {k: v.cuda().requires_grad_() for k, v in p.items()}
    l_got = loss_of(pg, "cuda", torch.float32, True)
    l_got.backward()
    assert abs(l_got.item() - l_ref.item()) < 1e-5 * l_ref.item()
    for k in p:
        assert rel_err(pg[k].grad.cpu(), pr[k].grad) < 1e-3, k
    opt = torch.optim.Adam(pg.values(), lr=1e-2)
    losses = []
    for _ in range(6):
        opt.zero_grad()
        loss = loss_of(pg, "cuda", torch.float32, True)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert losses[-1] < losses[0], losses
    # a 16-bit input: the op runs in fp32, the result comes back as x.dtype (to_dtype), the gradient too
    xh = x0.cuda().half().requires_grad_()
    y = cross_selective_scan(xh, *[pg[k].detach() for k in ("x_proj_weight",)], None,
                             *[pg[k].detach() for k in ("dt_projs_weight", "dt_projs_bias", "A_logs", "Ds")], None)
    assert y.dtype == torch.float16 and y.shape == (B, H, W, D)
    y.float().sum().backward()
    assert xh.grad.dtype == torch.float16
    with pytest.raises(RuntimeError, match="inconsistent shapes"):
        cross_selective_scan(x0.cuda(), pg["x_proj_weight"][:, :-1], None, pg["dt_projs_weight"], pg["dt_projs_bias"],
                             pg["A_logs"], pg["Ds"], None)


def test_memory_below_composition_at_down0():
    """down0, batch 2: the peak memory of one forward + backward of the fused op is below that of the reference-shaped
    composition (efficient_scan, the two einsums, selective_scan_train.selective_scan_fn, efficient_merge), same process.
    Measured on an MI355X (tools/cross_scan_train_bench.py): 850 MB against 1960 MB."""
    from founddiff_amd.selective_scan_train import selective_scan_fn
    p = {k: v.cuda().requires_grad_() for k, v in _params(128, 4, 4, seed=31).items()}
    x, dy = (t.cuda() for t in _x(2, 128, 512, 512, seed=32))

    def scan(u, delta, A, B, C, D, bias):
        return selective_scan_fn(u, delta, A, B, C, D, bias, delta_softplus=True)

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        xx = x.clone().requires_grad_()
        y = fn(xx, p)
        torch.autograd.grad(y, [xx] + [p[k] for k in PARAMS], dy)
        del y, xx
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    fused = peak(_fused)
    comp = peak(lambda xx, pp: _ref_y(xx, pp, scan))
    assert fused < comp, (fused, comp)
