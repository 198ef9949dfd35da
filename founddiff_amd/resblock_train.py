"""The reference's ResnetBlock (src/DADiff.py:397-430: one Block, src/DADiff.py:139-154, 213-229, plus a residual) for training:
the weight-standardised 3 x 3 convolution, GroupNorm, SiLU and the residual add as ONE autograd function on HIP kernels,
channel-last on both passes, exact fp32.

    out = block_core_fn(x, weight, bias, gn_weight, gn_bias, res)
        = SiLU(GroupNorm(conv3x3(x, weight) + bias)) + res

Forward: fd_conv2d(FD_F32) with GroupNorm partial sums in its epilogue -> h, fd_gn_finalize, fd_gn_silu_apply (+ res), exactly as
engine.res_block composes them.  Backward: fd_gn_silu_bwd_f32 (dout, h -> dh, dgamma, dbeta, dbias), fd_conv3x3_wgrad_f32 (x, dh ->
dweight), fd_conv2d(FD_F32) over dh with the mirrored, transposed weight -> dx; the gradient of res is dout itself.  Autograd keeps
x, the raw convolution output h and the GroupNorm statistics; no normalised copy, no SiLU input and no layout copy of an
activation exists on either pass.  Deterministic; a slice's out and gradient of x do not depend on the batch.  The weight
standardisation (at most 3.5 M elements) and the 1 x 1 res_conv stay with torch, the latter as F.linear on NHWC.

Binding for a training run:

    import DADiff, founddiff_amd.resblock_train as rbt
    DADiff.ResnetBlock.forward = rbt.resnet_block_forward

`ResnetBlock(dim, dim_out, *, time_emb_dim=None, groups=8)` is a module with the reference's parameter names and shapes (its
state dict loads with strict=True) for code that does not import the reference.
"""
import ctypes as C

import torch
import torch.nn.functional as F

from . import _lib as L
from ._train import HALF, cast_grads, check_devices, check_tensors, conv2d_f32, empty, f32, grad_out, ptr, stream, workspace
from ._train import strided as _strided

__all__ = ["block_core_fn", "ws_weight", "resnet_block_nhwc", "resnet_block_forward", "ResnetBlock"]

_SUPPORTED = ("Cin a multiple of 16, at most 1024; Cout a multiple of 32, at most 512; Cout % groups == 0 and (Cout / groups) "
              "% 4 == 0")


def _shape_ok(cin, cout, groups):
    return cin > 0 and cin % 16 == 0 and cin <= 1024 and cout > 0 and cout % 32 == 0 and cout <= 512 and groups > 0 and \
        cout % groups == 0 and (cout // groups) % 4 == 0


def _check_core(fn, x, weight, bias, gn_weight, gn_bias, res, groups):
    named = [("x", x), ("weight", weight), ("bias", bias), ("gn_weight", gn_weight), ("gn_bias", gn_bias), ("res", res)]
    check_tensors(fn, named, optional=("res",))
    shapes = " ".join(f"{n}{tuple(t.shape)}" for n, t in named if t is not None)
    if x.dim() != 4 or min(x.shape) < 1:
        raise RuntimeError(f"{fn}: inconsistent shapes {shapes} (x is (B, H, W, Cin))")
    if weight.dim() != 4 or tuple(weight.shape[1:]) != (x.shape[3], 3, 3):
        raise RuntimeError(f"{fn}: inconsistent shapes {shapes} (weight is (Cout, Cin, 3, 3))")
    cout = weight.shape[0]
    if any(tuple(t.shape) != (cout,) for t in (bias, gn_weight, gn_bias)):
        raise RuntimeError(f"{fn}: inconsistent shapes {shapes} (bias, gn_weight and gn_bias are (Cout,))")
    dims = (x.shape[0], x.shape[1], x.shape[2], cout)
    if res is not None and tuple(res.shape) != dims:
        raise RuntimeError(f"{fn}: inconsistent shapes {shapes} (res is (B, H, W, Cout) or None)")
    if not isinstance(groups, int) or not _shape_ok(x.shape[3], cout, groups):
        raise RuntimeError(f"{fn}: unsupported shape Cin={x.shape[3]} Cout={cout} groups={groups} ({_SUPPORTED})")
    check_devices(fn, named)
    return dims


class _BlockCore(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, gn_weight, gn_bias, res, groups, eps):
        args = (x, weight, bias, gn_weight, gn_bias, res)
        dims = B, H, W, cout = _check_core("block_core_fn", *args, groups)
        cin = x.shape[3]
        ctx.dtypes, ctx.dims, ctx.cin, ctx.groups = tuple(None if t is None else t.dtype for t in args), dims, cin, groups
        x, ld, off = _strided(f32(x), cin)
        w = f32(weight)
        bias, gamma, beta = (f32(t).contiguous() for t in (bias, gn_weight, gn_bias))
        r = None if res is None else f32(res).contiguous()
        dev = x.device
        with torch.cuda.device(dev):
            wk = w.permute(0, 2, 3, 1).contiguous()                     # [Cout][kh][kw][c], as fd_conv2d takes it
            mt = int(L.lib().fd_conv_mtiles(H, W))
            part = torch.empty(B, mt, cout, 2, device=dev, dtype=torch.float32)
            h = conv2d_f32(x, ld, off, cin, wk, bias, cout, (B, H, W), stats=part)
            del wk
            mr = torch.empty(B, groups, 2, device=dev, dtype=torch.float32)
            out = torch.empty(B, H, W, cout, device=dev, dtype=torch.float32)
            L.call("fd_gn_finalize", ptr(part), B, mt, cout, groups, H * W, float(eps), ptr(mr), stream(dev))
            L.call("fd_gn_silu_apply", L.FD_F32, ptr(h), ptr(mr), ptr(gamma), ptr(beta), ptr(r), ptr(out), B, H * W, cout, groups,
                   stream(dev))
        ctx.ld_off = (ld, off)
        ctx.save_for_backward(x, w, h, mr, gamma, beta)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, w, h, mr, gamma, beta = ctx.saved_tensors
        B, H, W, cout = ctx.dims
        cin, groups = ctx.cin, ctx.groups
        ld, off = ctx.ld_off
        dout = grad_out("block_core_fn", dout, ctx.dims)
        dev = x.device
        with torch.cuda.device(dev):
            new = empty(dev)
            dh, dgamma, dbeta, dbias = new(B, H, W, cout), new(cout), new(cout), new(cout)
            ws = workspace("fd_gn_silu_bwd_ws_floats", dev, B, H * W, cout, groups)
            L.call("fd_gn_silu_bwd_f32", ptr(dout), ptr(h), ptr(mr), ptr(gamma), ptr(beta), ptr(dh), ptr(dgamma), ptr(dbeta),
                   ptr(dbias), ptr(ws), B, H * W, cout, groups, stream(dev))
            dwk = new(cout, 3, 3, cin)
            ws = workspace("fd_conv3x3_wgrad_ws_floats", dev, B, H, W, cin, cout)
            L.call("fd_conv3x3_wgrad_f32", C.c_void_p(x.data_ptr() - 4 * off), ld, off, ptr(dh), ptr(dwk), ptr(ws), B, H, W, cin,
                   cout, stream(dev))
            del ws
            wd = w.flip(2, 3).permute(1, 2, 3, 0).contiguous()          # wd[c][kh][kw][n] = w[n][c][2 - kh][2 - kw]
            dx = conv2d_f32(dh, cout, 0, cout, wd, None, cin, (B, H, W))
            del dh, wd
        dres = dout if ctx.dtypes[5] is not None else None
        return cast_grads((dx, dwk.permute(0, 3, 1, 2), dbias, dgamma, dbeta, dres), ctx.dtypes) + (None, None)


def block_core_fn(x, weight, bias, gn_weight, gn_bias, res=None, groups=8, eps=1e-5):
    """(B, H, W, Cout) fp32 = SiLU(GroupNorm(conv3x3(x, weight) + bias)) + res, differentiable in every tensor argument.  x
    (B, H, W, Cin), dense or a channel slice of a dense wider tensor (read in place); weight (Cout, Cin, 3, 3) as torch holds it,
    already standardised by the caller; bias, gn_weight, gn_bias (Cout,); res (B, H, W, Cout) or None; eps the GroupNorm's.
    Cin a multiple of 16, at most 1024; Cout a multiple of 32, at most 512; Cout % groups == 0 and (Cout / groups) % 4 == 0:
    anything else raises RuntimeError("... unsupported shape ...").  16-bit tensors are up-cast; their gradients come back in
    their dtypes."""
    _check_core("block_core_fn", x, weight, bias, gn_weight, gn_bias, res, groups)
    return _BlockCore.apply(x, weight, bias, gn_weight, gn_bias, res, groups, eps)


def ws_weight(weight, eps=1e-5):
    """the weight standardisation of src/DADiff.py:145-152 (biased variance over all but the first axis), in torch"""
    mean = weight.mean(dim=(1, 2, 3), keepdim=True)
    var = weight.var(dim=(1, 2, 3), unbiased=False, keepdim=True)
    return (weight - mean) * (var + eps).rsqrt()


def _check_module(fn, self, x, channel_axis):
    """what the shipped constructor never builds, and x, before anything is launched"""
    block = getattr(self, "block1", None)
    proj, norm, rc = getattr(block, "proj", None), getattr(block, "norm", None), getattr(self, "res_conv", None)
    nn = torch.nn
    if not isinstance(proj, nn.Conv2d) or tuple(proj.kernel_size) != (3, 3) or tuple(proj.padding) != (1, 1) or \
            tuple(proj.stride) != (1, 1) or tuple(proj.dilation) != (1, 1) or proj.groups != 1 or \
            getattr(proj, "padding_mode", "zeros") != "zeros" or proj.bias is None:
        raise RuntimeError(f"{fn}: block1.proj must be a 3x3 convolution with padding 1, stride 1, dilation 1, groups 1, zero "
                           "padding and a bias")
    if not isinstance(norm, nn.GroupNorm) or not norm.affine:
        raise RuntimeError(f"{fn}: block1.norm must be an affine GroupNorm")
    cin, cout = proj.in_channels, proj.out_channels
    if isinstance(rc, nn.Conv2d):
        if tuple(rc.kernel_size) != (1, 1) or tuple(rc.stride) != (1, 1) or tuple(rc.padding) != (0, 0) or rc.groups != 1:
            raise RuntimeError(f"{fn}: res_conv must be a 1x1 convolution or nn.Identity")
        if rc.in_channels != cin or rc.out_channels != cout:
            raise RuntimeError(f"{fn}: inconsistent shapes: res_conv is {rc.in_channels} -> {rc.out_channels}, block1.proj {cin} -> "
                               f"{cout}")
    elif not isinstance(rc, nn.Identity):
        raise RuntimeError(f"{fn}: res_conv must be a 1x1 convolution or nn.Identity")
    elif cin != cout:
        raise RuntimeError(f"{fn}: inconsistent shapes: res_conv is nn.Identity, block1.proj {cin} -> {cout}")
    if norm.num_channels != cout:
        raise RuntimeError(f"{fn}: inconsistent shapes: block1.norm has {norm.num_channels} channels, block1.proj {cin} -> {cout}")
    if not _shape_ok(cin, cout, norm.num_groups):
        raise RuntimeError(f"{fn}: unsupported shape Cin={cin} Cout={cout} groups={norm.num_groups} ({_SUPPORTED})")
    if not isinstance(x, torch.Tensor):
        raise RuntimeError(f"{fn}: x must be a tensor (got {type(x).__name__})")
    if x.dtype not in (torch.float32,) + HALF:
        raise RuntimeError(f"{fn}: x must be float32 / float16 / bfloat16 (got {x.dtype})")
    if x.dim() != 4 or x.shape[channel_axis] != cin or min(x.shape) < 1:
        want = f"(B, {cin}, H, W)" if channel_axis == 1 else f"(B, H, W, {cin})"
        raise RuntimeError(f"{fn}: inconsistent shapes x{tuple(x.shape)} (expected {want})")
    for name, t in (("x", x), ("block1.proj.weight", proj.weight)):
        if not t.is_cuda:
            raise RuntimeError(f"{fn}: {name} must live on the GPU (there is no CPU path)")
    return cin, cout


def _nhwc(self, x, cin, cout):
    proj, norm, rc = self.block1.proj, self.block1.norm, self.res_conv
    w = ws_weight(proj.weight, 1e-5 if x.dtype == torch.float32 else 1e-3)
    res = x if isinstance(rc, torch.nn.Identity) else F.linear(x, rc.weight.view(cout, cin), rc.bias)
    return block_core_fn(x, w, proj.bias, norm.weight, norm.bias, res, norm.num_groups, norm.eps).to(x.dtype)


def resnet_block_nhwc(self, x):
    """ResnetBlock.forward on a channel-last x (B, H, W, dim) -> (B, H, W, dim_out) in x's dtype, with no layout copy.  Reads the
    reference's attribute names (block1.proj, block1.norm, res_conv); the weight standardisation (eps 1e-5 for a float32 x, 1e-3
    otherwise, as the reference) and a 1 x 1 res_conv (F.linear with weight.view(out, in)) stay with torch."""
    cin, cout = _check_module("resnet_block_nhwc", self, x, 3)
    return _nhwc(self, x, cin, cout)


def resnet_block_forward(self, x, time_emb=None):
    """ResnetBlock.forward (src/DADiff.py:418-430): x (B, dim, H, W) -> (B, dim_out, H, W) in x's dtype, a permute view of a
    channel-last tensor; time_emb is ignored, as in the reference.  An x whose permute(0, 2, 3, 1) is dense -- what a bound
    Mamba_block, torch's channels-last convolutions and torch.cat of such tensors hand over -- is used in place; any other x costs
    one NHWC copy.  Raises RuntimeError, before anything is launched, for a block1.proj that is not a 3 x 3 convolution with
    padding 1, stride 1, dilation 1, groups 1 and zero padding, a block1.norm that is not an affine GroupNorm, a res_conv that is
    neither a 1 x 1 convolution nor nn.Identity, unsupported channel counts, a CPU tensor, or inconsistent shapes."""
    cin, cout = _check_module("resnet_block_forward", self, x, 1)
    return _nhwc(self, x.permute(0, 2, 3, 1).contiguous(), cin, cout).permute(0, 3, 1, 2)


class _WSConv2d(torch.nn.Conv2d):
    """the reference's WeightStandardizedConv2d (src/DADiff.py:139-154), for code that calls block1.proj on its own"""

    def forward(self, x):
        w = ws_weight(self.weight, 1e-5 if x.dtype == torch.float32 else 1e-3)
        return F.conv2d(x, w, self.bias, self.stride, self.padding, self.dilation, self.groups)


class _Block(torch.nn.Module):
    def __init__(self, dim, dim_out, groups=8):
        super().__init__()
        self.proj = _WSConv2d(dim, dim_out, 3, padding=1)
        self.norm = torch.nn.GroupNorm(groups, dim_out)
        self.act = torch.nn.SiLU()


class ResnetBlock(torch.nn.Module):
    """The reference's ResnetBlock: block1.proj = a weight-standardised Conv2d(dim, dim_out, 3, padding 1), block1.norm =
    GroupNorm(groups, dim_out), res_conv = Conv2d(dim, dim_out, 1) or nn.Identity when dim == dim_out; time_emb_dim is accepted
    and unused, as in the reference.  Parameter names, shapes and initialisation are the reference's.  The forward takes NCHW;
    resnet_block_nhwc(module, x) is the channel-last form."""

    def __init__(self, dim, dim_out, *, time_emb_dim=None, groups=8):
        super().__init__()
        self.block1 = _Block(dim, dim_out, groups=groups)
        self.res_conv = torch.nn.Conv2d(dim, dim_out, 1) if dim != dim_out else torch.nn.Identity()

    forward = resnet_block_forward
