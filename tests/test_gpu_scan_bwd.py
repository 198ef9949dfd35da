"""selective_scan_train.bwd (include/founddiff_hip.h: fd_selective_scan_bwd_f32, csrc/fd_scan_bwd.hip) against float64
gradients: autograd through the CPU oracle's selective_scan_torch on a short sequence, the hand-written loop of
tests/scan_bwd_ref.py (run with torch on the GPU) everywhere else.

Gates: du, ddelta, dB, dC < 1e-5 (the project's fp32-against-fp64 gate) and dA, dD, ddelta_bias < 1e-4 (sums over batch x L),
rel_err = max abs error over the reference's max abs value.  Measured on an MI355X: 0.8e-7 .. 2.9e-7 for all seven outputs at
every shape below (the fp32 rounding floor).  tests/test_gpu_scan_bwd_cases.py covers the launcher's other forms."""
import sys

import pytest
import torch

from conftest import rel_err
from scan_bwd_cases import _inputs
from scan_bwd_ref import scan_grads_f64

pytestmark = pytest.mark.gpu

BLOCK_SHAPES = [(128, 4), (128, 8), (256, 16), (512, 32), (1024, 32), (512, 16), (256, 8)]     # (d_inner, d_state)
NAMES = ("du", "ddelta", "dA", "dB", "dC", "dD", "ddelta_bias")
GATES = dict(du=1e-5, ddelta=1e-5, dB=1e-5, dC=1e-5, dA=1e-4, dD=1e-4, ddelta_bias=1e-4)


def _check(got, ref, tag, errs=None):
    for name, x, y in zip(NAMES, got, ref):
        if y is None:
            assert x is None, (tag, name)
            continue
        assert x.shape == y.shape, (tag, name, x.shape, y.shape)
        e = rel_err(x.cpu(), y.cpu())
        if errs is not None:
            errs[name] = max(errs.get(name, 0.0), e)
        print(f"scan_bwd[{tag}] {name} {e:.3e}")
        assert e < GATES[name], f"{tag}: {name} error {e:.3e} >= {GATES[name]:.0e}"


def _run(m, u, delta, A, Bm, Cm, D, bias, dout, softplus, nrows=1):
    out, x = m.fwd(u, delta, A, Bm, Cm, D, bias, softplus, nrows)
    return m.bwd(u, delta, A, Bm, Cm, D, bias, dout, x, softplus, nrows)


def test_reference_loop_and_kernel_against_autograd():
    """The hand-written fp64 loop of scan_bwd_ref and the HIP backward against autograd through the CPU oracle's
    selective_scan_torch (float64), L = 37 over one partial tile, K = 2 groups.  The loop agrees to 2e-15 (CPU)."""
    from founddiff_amd import selective_scan_train as m
    from oracle import nets
    u, delta, A, Bm, Cm, D, bias, dout = _inputs(2, 16, 2, 3, 37, seed=1)
    leaves = [t.double().requires_grad_() for t in (u, delta, A, Bm, Cm, D, bias)]
    out = nets.selective_scan_torch(*leaves, softplus=True)
    ref = torch.autograd.grad(out, leaves, dout.double())
    loop = scan_grads_f64(u, delta, A, Bm, Cm, D, bias, dout, True, chunk=16)
    for name, x, y in zip(NAMES, loop, ref):
        assert rel_err(x, y) < 1e-12, name
    got = _run(m, *[t.cuda() for t in (u, delta, A, Bm, Cm, D, bias, dout)], True)
    _check(got, ref, "autograd")


@pytest.mark.parametrize("shape", BLOCK_SHAPES)
def test_every_block_shape(shape):
    """Every (d_inner, d_state) of the architecture's Mamba blocks with K = 4 groups (KD = 4 d_inner): L = 1029 (ragged,
    five tiles) with softplus, D and delta_bias; L = 37 without softplus, D and delta_bias, nrows = 2.  Measured on an
    MI355X: 0.8e-7 .. 2.9e-7 for every output at every shape (the deep levels split a group's rows over workgroups)."""
    from founddiff_amd import selective_scan_train as m
    d_inner, N = shape
    KD = 4 * d_inner
    u, delta, A, Bm, Cm, D, bias, dout = _inputs(2, KD, 4, N, 1029, seed=d_inner + N, device="cuda")
    got = _run(m, u, delta, A, Bm, Cm, D, bias, dout, True)
    _check(got, scan_grads_f64(u, delta, A, Bm, Cm, D, bias, dout, True), f"{shape} L=1029 softplus")
    u, delta, A, Bm, Cm, D, bias, dout = _inputs(2, KD, 4, N, 37, seed=d_inner + N + 1, device="cuda")
    delta = delta.abs() * 0.1
    got = _run(m, u, delta, A, Bm, Cm, None, None, dout, False, nrows=2)
    _check(got, scan_grads_f64(u, delta, A, Bm, Cm, None, None, dout, False), f"{shape} L=37 plain")


def test_three_dimensional_B_C():
    """B / C as (b, N, L), a single group: dB / dC come back 3-D."""
    from founddiff_amd import selective_scan_train as m
    u, delta, A, Bm, Cm, D, bias, dout = _inputs(2, 96, 1, 6, 1029, seed=3, device="cuda")
    got = _run(m, u, delta, A, Bm[:, 0], Cm[:, 0], D, bias, dout, True, nrows=2)
    assert got[3].shape == (2, 6, 1029) and got[4].shape == (2, 6, 1029)
    ref = scan_grads_f64(u, delta, A, Bm, Cm, D, bias, dout, True)
    _check(got, ref[:3] + (ref[3][:, 0], ref[4][:, 0]) + ref[5:], "3-D B/C")


@pytest.fixture(scope="module")
def level0():
    """the level-0 training shape of the reference (train.py: batch 2 at 512 x 512): KD = 512, K = 4, N = 4, L = 65536"""
    from founddiff_amd import selective_scan_train as m
    ins = _inputs(2, 512, 4, 4, 65536, seed=7, device="cuda")
    return ins, _run(m, *ins, True)


def test_long_sequence_level0(level0):
    """Level 0 against the fp64 loop (on the GPU): 256 tiles of carries.  Measured: du 1.2e-7, ddelta 1.4e-7, dA 1.7e-7,
    dB 2.2e-7, dC 1.9e-7, dD 1.0e-7, ddelta_bias 1.9e-7."""
    ins, got = level0
    ref = scan_grads_f64(*ins, True)
    _check(got, ref, "level 0")


def test_determinism_level0(level0):
    """A second call on the same inputs gives the same bits in all seven outputs (no float atomics)."""
    from founddiff_amd import selective_scan_train as m
    ins, got = level0
    again = _run(m, *ins, True)
    torch.cuda.synchronize()
    for name, x, y in zip(NAMES, got, again):
        assert torch.equal(x, y), name


def test_reference_call_pattern(monkeypatch):
    """src/emamba2.py:154 and 172 as written, with the module bound under the extension's name."""
    import founddiff_amd.selective_scan_train as train
    from founddiff_amd import selective_scan_cuda_core as core
    monkeypatch.setitem(sys.modules, "selective_scan_cuda_core", train)
    import selective_scan_cuda_core as m
    assert m.fwd is core.fwd
    u, delta, A, Bm, Cm, D, bias, dout = _inputs(2, 64, 4, 4, 300, seed=5, device="cuda")
    out, x, *rest = m.fwd(u, delta, A, Bm, Cm, D, bias, True, 1)
    du, ddelta, dA, dB, dC, dD, ddelta_bias, *rest = m.bwd(u, delta, A, Bm, Cm, D, bias, dout, x, True, 1)
    assert rest == []
    assert du.shape == ddelta.shape == u.shape and dA.shape == A.shape and dB.shape == Bm.shape and dC.shape == Cm.shape
    assert dD.shape == D.shape and ddelta_bias.shape == bias.shape
    assert all(t.device == u.device and t.dtype == torch.float32 for t in (du, ddelta, dA, dB, dC, dD, ddelta_bias))
    out, x, *rest = m.fwd(u, delta, A, Bm, Cm, None, None, True, 1)
    res = m.bwd(u, delta, A, Bm, Cm, None, None, dout, x, True, 1)
    assert len(res) == 7 and res[5] is None and res[6] is None
    # 16-bit inputs are up-cast like fwd's
    res16 = m.bwd(u.half(), delta.half(), A, Bm.bfloat16(), Cm.bfloat16(), D, bias, dout.half(), x, True, 1)
    assert all(t.dtype == torch.float32 for t in res16 if t is not None)


def test_ss2d_training_step():
    """An SS2D-shaped graph (x_proj and dt_proj einsums, A = -exp(A_logs), softplus scan with D and the dt bias, a scalar
    loss) through selective_scan_fn on the GPU against the same graph in float64 on the CPU through the oracle's
    selective_scan_torch; then a few Adam steps on the GPU lower the loss."""
    from founddiff_amd.selective_scan_train import selective_scan_fn
    from oracle import nets
    b, K, d, N, R, L = 2, 4, 32, 4, 8, 64
    g = torch.Generator().manual_seed(11)
    params = dict(
        x_proj_weight=torch.randn(K, R + 2 * N, d, generator=g) * d ** -0.5,
        dt_projs_weight=torch.randn(K, d, R, generator=g) * R ** -0.5,
        dt_projs_bias=torch.randn(K, d, generator=g) * 0.3 - 2,
        A_logs=torch.log(torch.arange(1, N + 1).float())[None].repeat(K * d, 1),
        Ds=torch.ones(K * d))
    xs0 = torch.randn(b, K, d, L, generator=g)
    target = torch.randn(b, K * d, L, generator=g)

    def loss_of(xs, p, scan):
        x_dbl = torch.einsum("bkdl,kcd->bkcl", xs, p["x_proj_weight"])
        dts, Bs, Cs = torch.split(x_dbl, [R, N, N], dim=2)
        dts = torch.einsum("bkrl,kdr->bkdl", dts, p["dt_projs_weight"])
        out = scan(xs.reshape(b, -1, L), dts.reshape(b, -1, L), -torch.exp(p["A_logs"]), Bs.contiguous(), Cs.contiguous(),
                   p["Ds"], p["dt_projs_bias"].reshape(-1))
        return ((out - target.to(out)) ** 2).mean()

    def grads(device, dtype, scan):
        p = {k: v.to(device, dtype).requires_grad_() for k, v in params.items()}
        xs = xs0.to(device, dtype).requires_grad_()
        loss = loss_of(xs, p, scan)
        loss.backward()
        return loss.detach(), xs.grad, {k: v.grad for k, v in p.items()}

    l_ref, gx_ref, gp_ref = grads("cpu", torch.float64, lambda *a: nets.selective_scan_torch(*a, softplus=True))
    l_got, gx_got, gp_got = grads("cuda", torch.float32, lambda *a: selective_scan_fn(*a, delta_softplus=True))
    assert abs(float(l_got) - float(l_ref)) < 1e-5 * float(l_ref)
    assert rel_err(gx_got.cpu(), gx_ref) < 1e-4
    for k in params:
        assert rel_err(gp_got[k].cpu(), gp_ref[k]) < 1e-3, k
    # training: Adam on the GPU
    p = {k: v.cuda().requires_grad_() for k, v in params.items()}
    xs = xs0.cuda()
    opt = torch.optim.Adam(p.values(), lr=1e-2)
    losses = []
    for _ in range(8):
        opt.zero_grad()
        loss = loss_of(xs, p, lambda *a: selective_scan_fn(*a, delta_softplus=True))
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert losses[-1] < losses[0], losses


def test_error_paths():
    """CPU tensors, a dout of the wrong shape and nrows = 5 raise RuntimeError with the library's message."""
    from founddiff_amd import selective_scan_train as m
    cpu = _inputs(2, 64, 4, 4, 100, seed=9)
    u, delta, A, Bm, Cm, D, bias, dout = [t.cuda() for t in cpu]
    out, x = m.fwd(u, delta, A, Bm, Cm, D, bias, True, 1)
    with pytest.raises(RuntimeError):
        m.bwd(*cpu[:7], cpu[7], x.cpu(), True, 1)
    with pytest.raises(RuntimeError):
        m.bwd(u, delta, A, Bm, Cm, D, bias, dout[:, :, :50].contiguous(), x, True, 1)
    with pytest.raises(RuntimeError, match="nrows"):
        m.bwd(u, delta, A, Bm, Cm, D, bias, dout, x, True, 5)
