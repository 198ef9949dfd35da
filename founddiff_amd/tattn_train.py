"""The reference's TransposedAttention (src/DADiff.py:252-285, Restormer channel attention) for training: everything between the
qkv GEMM and project_out as ONE autograd function on HIP kernels, channel-last on both passes.

    out = tattn_core_fn(qkv_pre, dw_weight, dw_bias, temperature)
        = chan_attn_fn(dwconv3x3(qkv_pre) + dw_bias, temperature)
    chan_attn_fn(qkv, temperature)[b, p, 32 h + i] = sum_j softmax_j(temperature[h] qhat_i . khat_j)[i, j] v[b, p, 32 h + j]

with q | k | v the thirds of qkv's channels, qhat / khat the columns of q / k L2-normalised over ALL pixels (F.normalize) and heads
of 32 channels (heads = dim // 32, as Mamba_block builds it).

Forward: fd_dwconv3x3 -> qkv, fd_chan_attn_fwd_f32 (a Gram pass over q and k, a 32 x 32 softmax per head, one pass v -> out).
Backward: fd_chan_attn_bwd_f32 (a Gram pass over dout and v, a per-head kernel, one pass q, k, dout -> dq | dk | dv) ->
fd_dwconv3x3_bwd_f32.  Autograd keeps qkv_pre (alive anyway as the qkv GEMM's output), qkv, and per (b, head) the softmax, the
normalised Gram and the 64 norms; no chunk, cat, normalised copy or layout copy of an activation exists on either pass.
Deterministic; a slice's out and gradient do not depend on the batch.  The two 1 x 1 convolutions (qkv, project_out) stay with
torch, as F.linear on NHWC.

Binding for a training run:

    import DADiff, founddiff_amd.tattn_train as tat
    DADiff.TransposedAttention.forward = tat.transposed_attention_forward

`TransposedAttention(dim, heads, bias=False)` is a module with the reference's parameter names and shapes (its state dict loads
with strict=True) for code that does not import the reference.
"""
import ctypes as C

import torch
import torch.nn.functional as F

from . import _lib as L
from ._train import cast_grads, check_devices, check_tensors, empty, f32, grad_out, ptr, stream, workspace
from ._train import strided as _strided

__all__ = ["chan_attn_fn", "tattn_core_fn", "transposed_attention_forward", "transposed_attention_nhwc", "TransposedAttention"]

def _check_dim(fn, C3, temperature, shapes):
    if C3 % 3:
        raise RuntimeError(f"{fn}: inconsistent shapes {shapes} (the last dimension is 3 dim: q | k | v)")
    dim = C3 // 3
    if temperature.numel() * 32 != dim or temperature.dim() not in (1, 3) or temperature.shape[0] != temperature.numel():
        raise RuntimeError(f"{fn}: inconsistent shapes {shapes} (temperature is (heads,) or (heads, 1, 1) with heads * 32 == dim = "
                           f"{dim}: heads are 32 channels wide)")
    if dim % 64 or dim > 512:
        raise RuntimeError(f"{fn}: unsupported shape dim={dim} (a multiple of 64, at most 512)")
    return dim


def _check_attn(fn, qkv, temperature):
    named = [("qkv", qkv), ("temperature", temperature)]
    check_tensors(fn, named)
    shapes = " ".join(f"{n}{tuple(t.shape)}" for n, t in named)
    if qkv.dim() != 4 or min(qkv.shape) < 1:
        raise RuntimeError(f"{fn}: inconsistent shapes {shapes} (qkv is (B, H, W, 3 dim))")
    dim = _check_dim(fn, qkv.shape[-1], temperature, shapes)
    check_devices(fn, named)
    return qkv.shape[0], qkv.shape[1], qkv.shape[2], dim


def _check_core(fn, qkv_pre, dw_weight, dw_bias, temperature):
    named = [("qkv_pre", qkv_pre), ("dw_weight", dw_weight), ("dw_bias", dw_bias), ("temperature", temperature)]
    check_tensors(fn, named, optional=("dw_bias",))
    shapes = " ".join(f"{n}{tuple(t.shape)}" for n, t in named if t is not None)
    if qkv_pre.dim() != 4 or min(qkv_pre.shape) < 1:
        raise RuntimeError(f"{fn}: inconsistent shapes {shapes} (qkv_pre is (B, H, W, 3 dim))")
    C3 = qkv_pre.shape[-1]
    if tuple(dw_weight.shape) != (C3, 1, 3, 3) or (dw_bias is not None and tuple(dw_bias.shape) != (C3,)):
        raise RuntimeError(f"{fn}: inconsistent shapes {shapes} (dw_weight is (3 dim, 1, 3, 3), dw_bias (3 dim,) or None)")
    dim = _check_dim(fn, C3, temperature, shapes)
    check_devices(fn, named)
    return qkv_pre.shape[0], qkv_pre.shape[1], qkv_pre.shape[2], dim


def _attn_fwd(qkv, ld, off, temp, dims):
    B, H, W, dim = dims
    dev = qkv.device
    heads = dim // 32
    new = empty(dev)
    out, attn, ghat, nrm = new(B, H, W, dim), new(B, heads, 32, 32), new(B, heads, 32, 32), new(B, heads, 64)
    ws = workspace("fd_chan_attn_fwd_ws_floats", dev, B, H * W, dim)
    L.call("fd_chan_attn_fwd_f32", C.c_void_p(qkv.data_ptr() - 4 * off), ld, off, ptr(temp), ptr(out), ptr(attn), ptr(ghat), ptr(nrm),
           ptr(ws), B, H * W, dim, stream(dev))
    return out, attn, ghat, nrm


def _attn_bwd(qkv, ld, off, temp, attn, ghat, nrm, dout, dims):
    B, H, W, dim = dims
    dev = qkv.device
    dqkv = torch.empty(B, H, W, 3 * dim, device=dev, dtype=torch.float32)
    dtemp = torch.empty(dim // 32, device=dev, dtype=torch.float32)
    ws = workspace("fd_chan_attn_bwd_ws_floats", dev, B, H * W, dim)
    L.call("fd_chan_attn_bwd_f32", C.c_void_p(qkv.data_ptr() - 4 * off), ld, off, ptr(temp), ptr(attn), ptr(ghat), ptr(nrm),
           ptr(dout), ptr(dqkv), 3 * dim, 0, ptr(dtemp), ptr(ws), B, H * W, dim, stream(dev))
    return dqkv, dtemp


class _ChanAttn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, temperature):
        dims = _check_attn("chan_attn_fn", qkv, temperature)
        ctx.dtypes, ctx.tshape, ctx.dims = (qkv.dtype, temperature.dtype), temperature.shape, dims
        qkv, ld, off = _strided(f32(qkv), 3 * dims[3])
        temp = f32(temperature).reshape(-1).contiguous()
        with torch.cuda.device(qkv.device):
            out, attn, ghat, nrm = _attn_fwd(qkv, ld, off, temp, dims)
        ctx.ld_off = (ld, off)
        ctx.save_for_backward(qkv, temp, attn, ghat, nrm)
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, temp, attn, ghat, nrm = ctx.saved_tensors
        dout = grad_out("chan_attn_fn", dout, ctx.dims)
        with torch.cuda.device(qkv.device):
            dqkv, dtemp = _attn_bwd(qkv, *ctx.ld_off, temp, attn, ghat, nrm, dout, ctx.dims)
        return cast_grads((dqkv, dtemp.view(ctx.tshape)), ctx.dtypes)


class _TattnCore(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv_pre, dw_weight, dw_bias, temperature):
        args = (qkv_pre, dw_weight, dw_bias, temperature)
        dims = B, H, W, dim = _check_core("tattn_core_fn", *args)
        ctx.dtypes, ctx.tshape, ctx.dims = tuple(None if t is None else t.dtype for t in args), temperature.shape, dims
        C3 = 3 * dim
        x = f32(qkv_pre).contiguous()
        w9 = f32(dw_weight).reshape(C3, 9).t().contiguous()             # [9][3 dim] tap-major, as fd_dwconv3x3 takes it
        bias = None if dw_bias is None else f32(dw_bias).contiguous()
        temp = f32(temperature).reshape(-1).contiguous()
        dev = x.device
        with torch.cuda.device(dev):
            qkv = torch.empty(B, H, W, C3, device=dev, dtype=torch.float32)
            L.call("fd_dwconv3x3", L.FD_F32, ptr(x), C3, 0, ptr(w9), ptr(bias), 0, ptr(qkv), C3, 0, B, H, W, C3, stream(dev))
            out, attn, ghat, nrm = _attn_fwd(qkv, C3, 0, temp, dims)
        ctx.save_for_backward(x, qkv, w9, bias, temp, attn, ghat, nrm)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, qkv, w9, bias, temp, attn, ghat, nrm = ctx.saved_tensors
        B, H, W, dim = ctx.dims
        C3 = 3 * dim
        dout = grad_out("tattn_core_fn", dout, ctx.dims)
        dev = x.device
        with torch.cuda.device(dev):
            new = empty(dev)
            dqkv, dtemp = _attn_bwd(qkv, C3, 0, temp, attn, ghat, nrm, dout, ctx.dims)
            del dout
            dx, dw9, db = new(B, H, W, C3), new(9, C3), (None if bias is None else new(C3))
            ws = workspace("fd_dwconv3x3_bwd_ws_floats", dev, B, H, W, C3)
            L.call("fd_dwconv3x3_bwd_f32", ptr(x), C3, 0, ptr(w9), ptr(bias), ptr(dqkv), ptr(dx), C3, 0, ptr(dw9), ptr(db), ptr(ws),
                   B, H, W, C3, stream(dev))
            del dqkv, ws
        return cast_grads((dx, dw9.t().reshape(C3, 1, 3, 3), db, dtemp.view(ctx.tshape)), ctx.dtypes)


def chan_attn_fn(qkv, temperature):
    """(B, H, W, dim) fp32, differentiable in both arguments.  qkv (B, H, W, 3 dim): q | k | v, dense or a channel slice of a
    dense wider tensor (read in place); temperature (heads,), (heads, 1, 1) or (heads * 1 * 1,) with heads = dim / 32.  16-bit
    tensors are up-cast; their gradients come back in their dtypes."""
    _check_attn("chan_attn_fn", qkv, temperature)
    return _ChanAttn.apply(qkv, temperature)


def tattn_core_fn(qkv_pre, dw_weight, dw_bias, temperature):
    """(B, H, W, dim) fp32, differentiable in every tensor argument.  qkv_pre (B, H, W, 3 dim): the qkv GEMM's output; dw_weight
    (3 dim, 1, 3, 3), dw_bias (3 dim,) or None: qkv_dwconv; temperature as chan_attn_fn takes it."""
    _check_core("tattn_core_fn", qkv_pre, dw_weight, dw_bias, temperature)
    return _TattnCore.apply(qkv_pre, dw_weight, dw_bias, temperature)


def _check_module(fn, self, x, channel_axis):
    """what the shipped constructor never builds, and x, before anything is launched"""
    qkv, dw, proj = self.qkv, self.qkv_dwconv, self.project_out
    dim = proj.in_channels
    if self.num_heads * 32 != dim:
        raise RuntimeError(f"{fn}: num_heads={self.num_heads}, dim={dim}: only heads of 32 channels are supported (num_heads * 32 == "
                           "dim, as Mamba_block builds them)")
    if dim % 64 or dim > 512:
        raise RuntimeError(f"{fn}: unsupported shape dim={dim} (a multiple of 64, at most 512)")
    if tuple(dw.kernel_size) != (3, 3) or tuple(dw.padding) != (1, 1) or dw.groups != dw.in_channels or \
            dw.in_channels != dw.out_channels or tuple(dw.stride) != (1, 1) or tuple(dw.dilation) != (1, 1) or \
            getattr(dw, "padding_mode", "zeros") != "zeros":
        raise RuntimeError(f"{fn}: qkv_dwconv must be a depthwise 3x3 convolution with padding 1, stride 1 and dilation 1")
    for conv, cin, cout, name in ((qkv, dim, 3 * dim, "qkv"), (proj, dim, dim, "project_out")):
        if tuple(conv.kernel_size) != (1, 1) or conv.in_channels != cin or conv.out_channels != cout or conv.groups != 1 or \
                tuple(conv.stride) != (1, 1):
            raise RuntimeError(f"{fn}: {name} must be a 1x1 convolution {cin} -> {cout}")
    if dw.in_channels != 3 * dim:
        raise RuntimeError(f"{fn}: inconsistent shapes: qkv_dwconv has {dw.in_channels} channels, project_out {dim} (expected 3 dim)")
    if not isinstance(x, torch.Tensor):
        raise RuntimeError(f"{fn}: x must be a tensor (got {type(x).__name__})")
    if x.dim() != 4 or x.shape[channel_axis] != dim:
        want = f"(B, {dim}, H, W)" if channel_axis == 1 else f"(B, H, W, {dim})"
        raise RuntimeError(f"{fn}: inconsistent shapes x{tuple(x.shape)} (expected {want})")
    if not x.is_cuda:
        raise RuntimeError(f"{fn}: x must live on the GPU (there is no CPU path)")
    return dim


def _nhwc(self, x, dim):
    qkv_pre = F.linear(x, self.qkv.weight.view(3 * dim, dim), self.qkv.bias)
    y = tattn_core_fn(qkv_pre, self.qkv_dwconv.weight, self.qkv_dwconv.bias, self.temperature)
    return F.linear(y.to(qkv_pre.dtype), self.project_out.weight.view(dim, dim), self.project_out.bias)


def transposed_attention_nhwc(self, x):
    """TransposedAttention.forward on a channel-last x (B, H, W, dim) -> (B, H, W, dim) in x's dtype, with no layout copy: what
    mamba_block_train.mamba_block_forward calls.  Reads the reference's attribute names (qkv, qkv_dwconv, project_out,
    temperature, num_heads); the two 1 x 1 convolutions run as F.linear with weight.view(out, in), biases passed through."""
    dim = _check_module("transposed_attention_nhwc", self, x, 3)
    return _nhwc(self, x, dim)


def transposed_attention_forward(self, x, c=None):
    """TransposedAttention.forward (src/DADiff.py:263-285): x (B, dim, H, W) -> (B, dim, H, W) in x's dtype; c is ignored, as in
    the reference.  NCHW in and out costs one NHWC copy of x on the way in and one NCHW copy of the result on the way out (the
    reference's Mamba_block pays the same two copies around this call; mamba_block_train.mamba_block_forward pays neither).
    Raises RuntimeError, before anything is launched, for num_heads * 32 != dim, dim % 64 != 0 or dim > 512, a qkv_dwconv that is
    not a depthwise 3 x 3 with padding 1, stride 1 and dilation 1, a CPU tensor, or inconsistent shapes."""
    dim = _check_module("transposed_attention_forward", self, x, 1)
    return _nhwc(self, x.permute(0, 2, 3, 1), dim).permute(0, 3, 1, 2).contiguous()


class TransposedAttention(torch.nn.Module):
    """The reference's TransposedAttention: temperature (heads, 1, 1) = 1, qkv = Conv2d(dim, 3 dim, 1), qkv_dwconv = Conv2d(3 dim,
    3 dim, 3, padding 1, groups 3 dim), project_out = Conv2d(dim, dim, 1); parameter names, shapes and initialisation are the
    reference's.  The forward takes NCHW; transposed_attention_nhwc(module, x) is the channel-last form."""

    def __init__(self, dim, heads, bias=False):
        super().__init__()
        nn = torch.nn
        self.num_heads = heads
        self.temperature = nn.Parameter(torch.ones(heads, 1, 1))
        self.qkv = nn.Conv2d(dim, dim * 3, kernel_size=1, bias=bias)
        self.qkv_dwconv = nn.Conv2d(dim * 3, dim * 3, kernel_size=3, stride=1, padding=1, groups=dim * 3, bias=bias)
        self.project_out = nn.Conv2d(dim, dim, kernel_size=1, bias=bias)

    forward = transposed_attention_forward
