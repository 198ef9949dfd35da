"""The element-wise frame of the reference's Mamba_block (src/DADiff.py:477-488) for training, as two autograd functions on HIP
kernels (csrc/fd_adaln_train.hip), channel-last on both passes:

    adaln_fn(x, gamma, beta, shift, scale, eps) = LayerNorm(x; gamma, beta, eps) * (1 + scale[:, None, None, :]) + shift[:, None, None, :]
    gate_residual_fn(x, y, gate)                = x + gate[:, None, None, :] * y

shift, scale and gate are the chunks of adaLN_modulation's (B, 6C) output and reach the kernels as the strided views they are.
Forward: one launch each.  Backward of adaln_fn: one pass over dout, x and the per-pixel (mean, rstd) that writes dx and the
partial sums behind dshift, dscale, dgamma and dbeta; of gate_residual_fn: one pass that writes dy and the partial sums of dgate --
the gradient of x is the incoming gradient itself, returned without a copy.  Autograd keeps x, the statistics (2 floats per
pixel) and views of scale, gamma and beta for adaln_fn, y and a view of gate for gate_residual_fn; the LayerNorm output and the
modulate temporaries are never stored.  Deterministic; a slice's results do not depend on the batch.

adaln_skip_fn is adaln_fn with x passed through as a second result: the gradient that reaches x along the residual path comes
back as that result's gradient and joins dx inside the one backward pass, so autograd never adds the two with a kernel of its
own.  mamba_block_train.mamba_block_forward is built on it.
"""
import torch

from . import _lib as L
from ._train import cast_grads, check_devices, check_tensors, empty, f32, grad_out, ptr, stream, workspace

__all__ = ["adaln_fn", "adaln_skip_fn", "gate_residual_fn"]


def _check_c(fn, C, shapes):
    if C % 64 or C > 512:
        raise RuntimeError(f"{fn}: unsupported shape {shapes} (C a multiple of 64, at most 512)")


def _check_adaln(fn, x, gamma, beta, shift, scale):
    named = [("x", x), ("gamma", gamma), ("beta", beta), ("shift", shift), ("scale", scale)]
    check_tensors(fn, named, optional=("gamma", "beta"))
    if (gamma is None) != (beta is None):
        raise RuntimeError(f"{fn}: gamma and beta must be given together or both be None (a LayerNorm without an affine)")
    shapes = " ".join(f"{n}{tuple(t.shape)}" for n, t in named if t is not None)
    if x.dim() != 4 or min(x.shape) < 1:
        raise RuntimeError(f"{fn}: inconsistent shapes {shapes} (x is (B, H, W, C))")
    B, H, W, C = x.shape
    if tuple(shift.shape) != (B, C) or tuple(scale.shape) != (B, C) or \
            (gamma is not None and (tuple(gamma.shape) != (C,) or tuple(beta.shape) != (C,))):
        raise RuntimeError(f"{fn}: inconsistent shapes {shapes} (shift and scale are (B, C), gamma and beta (C,) or None)")
    _check_c(fn, C, shapes)
    check_devices(fn, named)
    return B, H, W, C


def _check_gate(fn, x, y, gate):
    named = [("x", x), ("y", y), ("gate", gate)]
    check_tensors(fn, named)
    shapes = " ".join(f"{n}{tuple(t.shape)}" for n, t in named)
    if x.dim() != 4 or min(x.shape) < 1:
        raise RuntimeError(f"{fn}: inconsistent shapes {shapes} (x is (B, H, W, C))")
    B, H, W, C = x.shape
    if y.shape != x.shape or tuple(gate.shape) != (B, C):
        raise RuntimeError(f"{fn}: inconsistent shapes {shapes} (y is (B, H, W, C) as x, gate (B, C))")
    _check_c(fn, C, shapes)
    check_devices(fn, named)
    return B, H, W, C


def _rows(t, C):
    """(tensor, row stride) for the kernels: t (B, C) itself if it is C columns of a dense wider matrix, else a dense copy"""
    t = f32(t)
    ld = t.stride(0)
    if t.stride(1) == 1 and ld >= C and ld % 4 == 0 and t.data_ptr() % 16 == 0:
        return t, ld
    return t.contiguous(), C


class _AdaLN(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, shift, scale, eps):
        args = (x, gamma, beta, shift, scale)
        dims = B, H, W, C = _check_adaln("adaln_fn", *args)
        ctx.dtypes, ctx.dims, ctx.eps = tuple(None if t is None else t.dtype for t in args), dims, float(eps)
        ctx.set_materialize_grads(False)
        xf = f32(x).contiguous()
        gm, bt = (None, None) if gamma is None else (f32(gamma).contiguous(), f32(beta).contiguous())
        sc, ld = _rows(scale, C)
        sh, ld_sh = _rows(shift, C)
        if ld_sh != ld:
            sc, sh, ld = sc.contiguous(), sh.contiguous(), C
        dev = xf.device
        with torch.cuda.device(dev):
            new = empty(dev)
            out, stats = new(B, H, W, C), new(B, H, W, 2)
            L.call("fd_adaln_fwd_f32", ptr(xf), ptr(gm), ptr(bt), ctx.eps, ptr(sh), ptr(sc), ld, ptr(out), ptr(stats), B, H * W, C,
                   stream(dev))
        ctx.ld = ld
        ctx.save_for_backward(xf, stats, sc, gm, bt)
        return out, x

    @staticmethod
    def backward(ctx, dout, dskip):
        if dout is None and dskip is None:
            return (None,) * 6
        xf, stats, sc, gm, bt = ctx.saved_tensors
        B, H, W, C = ctx.dims
        dev = xf.device
        if dout is None:                                                 # only the skip is used: dx is its gradient, no launch
            zc, zm = None if gm is None else torch.zeros(C, device=dev), torch.zeros(B, C, device=dev)
            return cast_grads((grad_out("adaln_fn", dskip, ctx.dims), zc, zc, zm, zm), ctx.dtypes) + (None,)
        dout = grad_out("adaln_fn", dout, ctx.dims)
        dres = None if dskip is None else grad_out("adaln_fn", dskip, ctx.dims)
        # needs_input_grad is not consulted: the sums behind the four small gradients ride on the pass that writes dx, and the
        # finishing kernel and its (C,) / (B, 2C) outputs cost microseconds, so frozen parameters take the same path
        with torch.cuda.device(dev):
            new = empty(dev)
            dx, dmod = new(B, H, W, C), new(B, 2 * C)                    # dshift | dscale
            dgm, dbt = (None, None) if gm is None else (new(C), new(C))
            ws = workspace("fd_adaln_bwd_ws_floats", dev, B, H * W, C)
            L.call("fd_adaln_bwd_f32", ptr(dout), ptr(xf), ptr(stats), ptr(gm), ptr(bt), ptr(sc), ctx.ld, ptr(dres), ptr(dx),
                   ptr(dmod), ptr(dmod[:, C:]), 2 * C, ptr(dgm), ptr(dbt), ptr(ws), B, H * W, C, stream(dev))
        return cast_grads((dx, dgm, dbt, dmod[:, :C], dmod[:, C:]), ctx.dtypes) + (None,)


class _GateRes(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, gate):
        dims = B, H, W, C = _check_gate("gate_residual_fn", x, y, gate)
        ctx.dtypes, ctx.dims = (x.dtype, y.dtype, gate.dtype), dims
        xf, yf = f32(x).contiguous(), f32(y).contiguous()
        gt, ld = _rows(gate, C)
        dev = xf.device
        with torch.cuda.device(dev):
            out = torch.empty(B, H, W, C, device=dev, dtype=torch.float32)
            L.call("fd_gate_res_fwd_f32", ptr(xf), ptr(yf), ptr(gt), ld, ptr(out), B, H * W, C, stream(dev))
        ctx.ld = ld
        ctx.save_for_backward(yf, gt)
        return out

    @staticmethod
    def backward(ctx, dout):
        yf, gt = ctx.saved_tensors
        B, H, W, C = ctx.dims
        dev = yf.device
        dx = dout                                                        # the gradient of x: no copy
        dout = grad_out("gate_residual_fn", dout, ctx.dims)
        with torch.cuda.device(dev):
            new = empty(dev)
            dy, dgate = new(B, H, W, C), new(B, C)
            ws = workspace("fd_gate_res_bwd_ws_floats", dev, B, H * W, C)
            L.call("fd_gate_res_bwd_f32", ptr(dout), ptr(yf), ptr(gt), ctx.ld, ptr(dy), ptr(dgate), C, ptr(ws), B, H * W, C,
                   stream(dev))
        return cast_grads((dx, dy, dgate), ctx.dtypes)


def adaln_skip_fn(x, gamma, beta, shift, scale, eps=1e-5):
    """(adaln_fn(...), x): the second result is x passed through, for the residual add behind the branch.  Its gradient is
    added to dx inside fd_adaln_bwd_f32 (dres); an unused second result costs nothing."""
    _check_adaln("adaln_fn", x, gamma, beta, shift, scale)
    return _AdaLN.apply(x, gamma, beta, shift, scale, eps)


def adaln_fn(x, gamma, beta, shift, scale, eps=1e-5):
    """(B, H, W, C) fp32, differentiable in every tensor argument.  x (B, H, W, C); gamma, beta (C,), or both None for a
    LayerNorm without an affine; shift, scale (B, C), dense or column ranges of a wider matrix (read in place); eps the
    LayerNorm's.  C a multiple of 64, at most 512.  16-bit tensors are up-cast; their gradients come back in their dtypes."""
    return adaln_skip_fn(x, gamma, beta, shift, scale, eps)[0]


def gate_residual_fn(x, y, gate):
    """x + gate[:, None, None, :] * y, (B, H, W, C) fp32, differentiable in all three arguments.  x, y (B, H, W, C); gate
    (B, C), dense or a column range of a wider matrix (read in place).  The gradient of x is the incoming gradient itself.
    16-bit tensors are up-cast; their gradients come back in their dtypes."""
    _check_gate("gate_residual_fn", x, y, gate)
    return _GateRes.apply(x, y, gate)
