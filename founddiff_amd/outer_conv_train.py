"""The two outer convolutions of the reference's Unet (src/DADiff.py:553-555 init_conv, 681 final_conv) for training: two autograd
functions on HIP kernels (csrc/fd_outer_train.hip), exact fp32.

    init_conv_fn(x, weight, bias)    Conv2d(Cin, Cout, 7, padding=3) of NCHW planes, Cin 2 or 3 -> (B, H, W, Cout) channel-last
    final_conv_fn(x, weight, bias)   Conv2d(C, 1, 1) of a channel-last x (B, H, W, C) -> (B, 1, H, W)

                 forward                          backward
    init_conv    fd_init_conv7_fwd_f32            fd_init_conv7_wgrad_f32: dweight and dbias in one pass over dout; x is data
    final_conv   fd_final_conv1_fwd_f32           fd_final_conv1_bwd_f32: dx, dweight and dbias in one pass over x and dout

Deterministic: no float atomics, fixed summation orders, no host synchronisation; a slice's out and dx do not depend on the batch.
There is no CPU path.

Binding: unet_train.unet_trunk_forward(..., init_fn=init_conv_fn, final_fn=final_conv_fn), as DADiff.Unet.train_forward calls it.
"""
import ctypes as C

import torch

from . import _lib as L
from ._train import cast_grads, check_devices, check_tensors, f32, grad_out, ptr, stream, strided, workspace

__all__ = ["init_conv_fn", "final_conv_fn"]


def _check_init(fn, x, weight, bias):
    named = [("x", x), ("weight", weight), ("bias", bias)]
    check_tensors(fn, named)
    shapes = " ".join(f"{n}{tuple(t.shape)}" for n, t in named)
    if x.dim() != 4 or min(x.shape) < 1:
        raise RuntimeError(f"{fn}: inconsistent shapes {shapes} (x is (B, Cin, H, W))")
    if weight.dim() != 4 or tuple(weight.shape[1:]) != (x.shape[1], 7, 7):
        raise RuntimeError(f"{fn}: inconsistent shapes {shapes} (weight is (Cout, Cin, 7, 7))")
    cout = weight.shape[0]
    if tuple(bias.shape) != (cout,):
        raise RuntimeError(f"{fn}: inconsistent shapes {shapes} (bias is (Cout,))")
    if x.shape[1] not in (2, 3) or cout < 1 or cout % 32 or cout > 512:
        raise RuntimeError(f"{fn}: unsupported shape Cin={x.shape[1]} Cout={cout} (Cin 2 or 3, Cout a multiple of 32, at most 512)")
    if x.shape[0] > 65535 or max(x.shape[2:]) > 32768:
        raise RuntimeError(f"{fn}: unsupported shape {shapes} (at most 65535 slices of at most 32768 x 32768)")
    check_devices(fn, named)
    if x.requires_grad:
        raise RuntimeError(f"{fn}: x is data: it must not require a gradient (the input gradient of init_conv is not built)")
    return x.shape[0], x.shape[1], x.shape[2], x.shape[3], cout


class _Init(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias):
        B, cin, H, W, cout = ctx.dims = _check_init("init_conv_fn", x, weight, bias)
        ctx.dtypes = (weight.dtype, bias.dtype)
        x, w, b = f32(x).contiguous(), f32(weight).contiguous(), f32(bias).contiguous()
        dev = x.device
        with torch.cuda.device(dev):
            out = torch.empty(B, H, W, cout, device=dev, dtype=torch.float32)
            L.call("fd_init_conv7_fwd_f32", ptr(x), ptr(w), ptr(b), ptr(out), B, cin, H, W, cout, stream(dev))
        ctx.save_for_backward(x)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, = ctx.saved_tensors
        B, cin, H, W, cout = ctx.dims
        dout = grad_out("init_conv_fn", dout, (B, H, W, cout))
        dev = x.device
        with torch.cuda.device(dev):
            g = torch.empty(49 * cin + 1, cout, device=dev, dtype=torch.float32)
            ws = workspace("fd_init_conv7_wgrad_ws_floats", dev, B, cin, H, W, cout)
            L.call("fd_init_conv7_wgrad_f32", ptr(x), ptr(dout), ptr(g), ptr(ws), B, cin, H, W, cout, stream(dev))
            dw = g[:49 * cin].view(cin, 7, 7, cout).permute(3, 0, 1, 2).contiguous()
            db = g[49 * cin].clone()
        return (None,) + cast_grads((dw, db), ctx.dtypes)


def init_conv_fn(x, weight, bias):
    """(B, H, W, Cout) fp32 channel-last = Conv2d(Cin, Cout, 7, padding=3) of x (B, Cin, H, W), dense NCHW planes, Cin 2 or 3.
    weight (Cout, Cin, 7, 7) as torch holds it, bias (Cout,); Cout a multiple of 32, at most 512.  Differentiable in weight and
    bias.  x is data: an x that requires a gradient raises RuntimeError in forward.  Anything unsupported raises RuntimeError
    before a launch.  16-bit tensors are up-cast; their gradients come back in their dtypes."""
    _check_init("init_conv_fn", x, weight, bias)
    return _Init.apply(x, weight, bias)


def _check_final(fn, x, weight, bias):
    named = [("x", x), ("weight", weight), ("bias", bias)]
    check_tensors(fn, named)
    shapes = " ".join(f"{n}{tuple(t.shape)}" for n, t in named)
    if x.dim() != 4 or min(x.shape) < 1:
        raise RuntimeError(f"{fn}: inconsistent shapes {shapes} (x is (B, H, W, C))")
    if tuple(weight.shape) != (1, x.shape[3], 1, 1) or tuple(bias.shape) != (1,):
        raise RuntimeError(f"{fn}: inconsistent shapes {shapes} (weight is (1, C, 1, 1), bias (1,))")
    c = x.shape[3]
    if c % 4 or c > 1024:
        raise RuntimeError(f"{fn}: unsupported shape C={c} (a multiple of 4, at most 1024)")
    if x.shape[0] * x.shape[1] * x.shape[2] > 1 << 30:
        raise RuntimeError(f"{fn}: unsupported shape {shapes} (at most 2^30 pixels)")
    check_devices(fn, named)
    return x.shape[0], x.shape[1], x.shape[2], c


class _Final(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias):
        B, H, W, c = ctx.dims = _check_final("final_conv_fn", x, weight, bias)
        ctx.dtypes = (x.dtype, weight.dtype, bias.dtype)
        x, ld, off = strided(f32(x), c)
        w, b = f32(weight).contiguous().view(c), f32(bias).contiguous()
        dev = x.device
        with torch.cuda.device(dev):
            out = torch.empty(B, 1, H, W, device=dev, dtype=torch.float32)
            L.call("fd_final_conv1_fwd_f32", C.c_void_p(x.data_ptr() - 4 * off), ld, off, ptr(w), ptr(b), ptr(out), B * H * W, c,
                   stream(dev))
        ctx.ld_off = (ld, off)
        ctx.save_for_backward(x, w)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, w = ctx.saved_tensors
        B, H, W, c = ctx.dims
        ld, off = ctx.ld_off
        dout = grad_out("final_conv_fn", dout, (B, 1, H, W))
        dev = x.device
        with torch.cuda.device(dev):
            dx = torch.empty(B, H, W, c, device=dev, dtype=torch.float32)
            dwb = torch.empty(c + 4, device=dev, dtype=torch.float32)
            ws = workspace("fd_final_conv1_bwd_ws_floats", dev, B * H * W, c)
            L.call("fd_final_conv1_bwd_f32", C.c_void_p(x.data_ptr() - 4 * off), ld, off, ptr(w), ptr(dout), ptr(dx), ptr(dwb), ptr(ws),
                   B * H * W, c, stream(dev))
            dw, db = dwb[:c].clone().view(1, c, 1, 1), dwb[c:c + 1].clone()
        return cast_grads((dx, dw, db), ctx.dtypes)


def final_conv_fn(x, weight, bias):
    """(B, 1, H, W) fp32 = Conv2d(C, 1, 1) of a channel-last x (B, H, W, C), dense or a channel slice of a dense wider tensor (read
    in place); differentiable in all three.  weight (1, C, 1, 1), bias (1,); C a multiple of 4, at most 1024.  Anything unsupported
    raises RuntimeError before a launch.  16-bit tensors are up-cast; their gradients come back in their dtypes."""
    _check_final("final_conv_fn", x, weight, bias)
    return _Final.apply(x, weight, bias)
