"""The eight convolutions of the reference's Unet (src/DADiff.py:530-740) that change resolution or close a level, for training:
three autograd functions on HIP kernels, channel-last on both passes, exact fp32.

    downsample_fn(x, weight, bias)   Conv2d(4, stride 2, padding 1)                 src/DADiff.py:135-136
    upsample_fn(x, weight, bias)     nearest x2 -> Conv2d(3, padding 1)             src/DADiff.py:128-132
    conv3x3_fn(x, weight, bias)      Conv2d(3, padding 1)                           src/DADiff.py:642-643, 674-675

Write Down for the first and Up for the second.  Output pixel (2i+a, 2j+b) of Up reads source pixels (i+a+r-1, j+b+s-1), r, s in
{0, 1}, with the 3x3 taps that land on one source pixel summed; the input gradient of Down has the same index map with no
summing.  So Up(x, w) is the transpose of Down with the folded 4x4 kernel w4 = up_weight_4x4(w), and

                 forward                          dx                                      dweight
    Down         fd_conv2d(4x4 / 2 / 1)           fd_conv_sub2x_f32(dout, w)              fd_corr4x4s2_f32(dout, x)
    Up           fd_conv_sub2x_f32(x, w4)         fd_conv2d(4x4 / 2 / 1)(dout, w4^T)      fd_corr4x4s2_f32(x, dout), unfolded
    3x3          fd_conv2d(3x3 / 1 / 1)           fd_conv2d on the mirrored w^T           fd_conv3x3_wgrad_f32

The nearest-upsampled tensor never exists, the Up products take 4 MACs per output where the 3x3 on the fine grid takes 9 (2.25 x
fewer in the weight gradient), and autograd keeps x and the weight alone.  Deterministic; a slice's out and gradient of x do not
depend on the batch.  The folds, unfolds and transposes of weights (at most 2 M elements) and dbias = dout.sum((0, 1, 2)) stay with
torch.

Binding: unet_train.unet_forward calls resample_nhwc(module, x) on the reference's three module forms.
"""
import ctypes as C

import torch

from . import _lib as L
from ._train import HALF, cast_grads, check_devices, check_tensors, conv2d_f32, f32, grad_out, ptr, stream, strided, workspace

__all__ = ["downsample_fn", "upsample_fn", "conv3x3_fn", "resample_nhwc", "up_weight_4x4", "up_weight_unfold", "sub2x_weight"]

_SUPPORTED = "Cin and Cout multiples of 32, at most 512"
# the 4x4 tap of sub-pixel (a, r): kh(0,0) = 3, kh(0,1) = 1, kh(1,0) = 2, kh(1,1) = 0
_TAP = (3, 1, 2, 0)


def _fold4(w, dim):
    k0, k1, k2 = w.unbind(dim)
    return torch.stack((k2, k1 + k2, k0 + k1, k0), dim)


def _unfold4(g, dim):
    t0, t1, t2, t3 = g.unbind(dim)
    return torch.stack((t2 + t3, t1 + t2, t0 + t1), dim)


def up_weight_4x4(weight):
    """(Cout, Cin, 3, 3) -> w4 (Cout, Cin, 4, 4), the 4x4 / stride 2 / padding 1 kernel whose transposed convolution is nearest x2
    followed by the 3x3 convolution: t = 0 <- kh 2, t = 1 <- kh 1 + 2, t = 2 <- kh 0 + 1, t = 3 <- kh 0; columns likewise"""
    return _fold4(_fold4(weight, 2), 3)


def up_weight_unfold(g4):
    """the transpose of up_weight_4x4: (..., 4, 4) -> (..., 3, 3), out[kh][kw] = the sum of g4[t][u] over t in {2 - kh, 3 - kh},
    u in {2 - kw, 3 - kw}"""
    return _unfold4(_unfold4(g4, -2), -1)


def sub2x_weight(w4):
    """w4 (N, C, 4, 4), a 4x4 / stride 2 / padding 1 kernel read as the weight of a TRANSPOSED convolution C -> N, -> w2
    [N][4][2][2][C] as fd_conv_sub2x_f32 takes it: w2[n][2a+b][r][s][c] = w4[n][c][kh(a,r)][kw(b,s)]"""
    N, Cc = w4.shape[:2]
    rows = w4.unbind(2)
    cols = torch.stack([rows[i] for i in _TAP], 2).unbind(3)
    w = torch.stack([cols[i] for i in _TAP], 3).reshape(N, Cc, 2, 2, 2, 2)                 # [n][c][a][r][b][s]
    return w.permute(0, 2, 4, 3, 5, 1).reshape(N, 4, 2, 2, Cc).contiguous()


def _shape_ok(cin, cout):
    return cin > 0 and cin % 32 == 0 and cin <= 512 and cout > 0 and cout % 32 == 0 and cout <= 512


def _check_fn(fn, x, weight, bias, k, even=False):
    named = [("x", x), ("weight", weight), ("bias", bias)]
    check_tensors(fn, named)
    shapes = " ".join(f"{n}{tuple(t.shape)}" for n, t in named)
    if x.dim() != 4 or min(x.shape) < 1:
        raise RuntimeError(f"{fn}: inconsistent shapes {shapes} (x is (B, H, W, Cin))")
    if weight.dim() != 4 or tuple(weight.shape[1:]) != (x.shape[3], k, k):
        raise RuntimeError(f"{fn}: inconsistent shapes {shapes} (weight is (Cout, Cin, {k}, {k}))")
    cout = weight.shape[0]
    if tuple(bias.shape) != (cout,):
        raise RuntimeError(f"{fn}: inconsistent shapes {shapes} (bias is (Cout,))")
    if not _shape_ok(x.shape[3], cout):
        raise RuntimeError(f"{fn}: unsupported shape Cin={x.shape[3]} Cout={cout} ({_SUPPORTED})")
    if even and (x.shape[1] % 2 or x.shape[2] % 2):
        raise RuntimeError(f"{fn}: unsupported shape H={x.shape[1]} W={x.shape[2]} (both must be even)")
    check_devices(fn, named)
    return x.shape[0], x.shape[1], x.shape[2], x.shape[3], cout


def _sub2x(x, w2, bias, dims, cin, cout):
    B, H, W = dims
    out = torch.empty(B, 2 * H, 2 * W, cout, device=x.device, dtype=torch.float32)
    L.call("fd_conv_sub2x_f32", ptr(x), ptr(w2), ptr(bias), ptr(out), B, H, W, cin, cout, stream(x.device))
    return out


def _corr(coarse, fine, dims, P, Q):
    """g [P][4][4][Q]; coarse (B, H, W, P), fine (B, 2H, 2W, Q)"""
    B, H, W = dims
    g = torch.empty(P, 4, 4, Q, device=coarse.device, dtype=torch.float32)
    ws = workspace("fd_corr4x4s2_ws_floats", coarse.device, B, H, W, P, Q)
    L.call("fd_corr4x4s2_f32", ptr(coarse), ptr(fine), ptr(g), ptr(ws), B, H, W, P, Q, stream(coarse.device))
    return g


class _Down(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias):
        B, H, W, cin, cout = _check_fn("downsample_fn", x, weight, bias, 4, even=True)
        ctx.dtypes, ctx.dims = (x.dtype, weight.dtype, bias.dtype), (B, H, W, cin, cout)
        x, w, bias = f32(x).contiguous(), f32(weight), f32(bias).contiguous()
        with torch.cuda.device(x.device):
            wk = w.permute(0, 2, 3, 1).contiguous()                     # [Cout][kh][kw][c], as fd_conv2d takes it
            out = conv2d_f32(x, cin, 0, cin, wk, bias, cout, (B, H, W), 4, 2)
        ctx.save_for_backward(x, w)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, w = ctx.saved_tensors
        B, H, W, cin, cout = ctx.dims
        dout = grad_out("downsample_fn", dout, (B, H // 2, W // 2, cout))
        with torch.cuda.device(x.device):
            w2 = sub2x_weight(w.transpose(0, 1))                        # [c][2a+b][r][s][n] = w[n][c][kh(a,r)][kw(b,s)]
            dx = _sub2x(dout, w2, None, (B, H // 2, W // 2), cout, cin)
            del w2
            g = _corr(dout, x, (B, H // 2, W // 2), cout, cin)          # [n][kh][kw][c]
            dbias = dout.sum((0, 1, 2))
        return cast_grads((dx, g.permute(0, 3, 1, 2), dbias), ctx.dtypes)


class _Up(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias):
        B, H, W, cin, cout = _check_fn("upsample_fn", x, weight, bias, 3)
        ctx.dtypes, ctx.dims = (x.dtype, weight.dtype, bias.dtype), (B, H, W, cin, cout)
        x, w, bias = f32(x).contiguous(), f32(weight), f32(bias).contiguous()
        with torch.cuda.device(x.device):
            w2 = sub2x_weight(up_weight_4x4(w))
            out = _sub2x(x, w2, bias, (B, H, W), cin, cout)
        ctx.save_for_backward(x, w)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, w = ctx.saved_tensors
        B, H, W, cin, cout = ctx.dims
        dout = grad_out("upsample_fn", dout, (B, 2 * H, 2 * W, cout))
        with torch.cuda.device(x.device):
            wd = up_weight_4x4(w).permute(1, 2, 3, 0).contiguous()      # wd[c][t][u][n]: Down-shaped, dout -> dx
            dx = conv2d_f32(dout, cout, 0, cout, wd, None, cin, (B, 2 * H, 2 * W), 4, 2)
            del wd
            g = _corr(x, dout, (B, H, W), cin, cout)                    # [c][t][u][n]
            dw = up_weight_unfold(g.permute(3, 0, 1, 2))
            dbias = dout.sum((0, 1, 2))
        return cast_grads((dx, dw, dbias), ctx.dtypes)


class _Conv3(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias):
        B, H, W, cin, cout = _check_fn("conv3x3_fn", x, weight, bias, 3)
        ctx.dtypes, ctx.dims = (x.dtype, weight.dtype, bias.dtype), (B, H, W, cin, cout)
        x, ld, off = strided(f32(x), cin)
        w, bias = f32(weight), f32(bias).contiguous()
        with torch.cuda.device(x.device):
            wk = w.permute(0, 2, 3, 1).contiguous()
            out = conv2d_f32(x, ld, off, cin, wk, bias, cout, (B, H, W), 3, 1)
        ctx.ld_off = (ld, off)
        ctx.save_for_backward(x, w)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, w = ctx.saved_tensors
        B, H, W, cin, cout = ctx.dims
        ld, off = ctx.ld_off
        dout = grad_out("conv3x3_fn", dout, (B, H, W, cout))
        dev = x.device
        with torch.cuda.device(dev):
            dwk = torch.empty(cout, 3, 3, cin, device=dev, dtype=torch.float32)
            ws = workspace("fd_conv3x3_wgrad_ws_floats", dev, B, H, W, cin, cout)
            L.call("fd_conv3x3_wgrad_f32", C.c_void_p(x.data_ptr() - 4 * off), ld, off, ptr(dout), ptr(dwk), ptr(ws), B, H, W, cin,
                   cout, stream(dev))
            del ws
            wd = w.flip(2, 3).permute(1, 2, 3, 0).contiguous()          # wd[c][kh][kw][n] = w[n][c][2 - kh][2 - kw]
            dx = conv2d_f32(dout, cout, 0, cout, wd, None, cin, (B, H, W), 3, 1)
            dbias = dout.sum((0, 1, 2))
        return cast_grads((dx, dwk.permute(0, 3, 1, 2), dbias), ctx.dtypes)


def downsample_fn(x, weight, bias):
    """(B, H/2, W/2, Cout) fp32 = Conv2d(4, stride 2, padding 1) of a channel-last x (B, H, W, Cin), differentiable in all three.
    weight (Cout, Cin, 4, 4) as torch holds it, bias (Cout,).  Cin and Cout multiples of 32, at most 512, H and W even: anything
    else raises RuntimeError("... unsupported shape ...").  16-bit tensors are up-cast; their gradients come back in their
    dtypes."""
    _check_fn("downsample_fn", x, weight, bias, 4, even=True)
    return _Down.apply(x, weight, bias)


def upsample_fn(x, weight, bias):
    """(B, 2H, 2W, Cout) fp32 = Conv2d(3, padding 1) of the nearest x2 up-sampling of a channel-last x (B, H, W, Cin), which is
    never built; differentiable in all three.  weight (Cout, Cin, 3, 3), bias (Cout,); channel counts and dtypes as
    downsample_fn."""
    _check_fn("upsample_fn", x, weight, bias, 3)
    return _Up.apply(x, weight, bias)


def conv3x3_fn(x, weight, bias):
    """(B, H, W, Cout) fp32 = Conv2d(3, padding 1) of a channel-last x (B, H, W, Cin), dense or a channel slice of a dense wider
    tensor (read in place); differentiable in all three.  weight (Cout, Cin, 3, 3), bias (Cout,); channel counts and dtypes as
    downsample_fn."""
    _check_fn("conv3x3_fn", x, weight, bias, 3)
    return _Conv3.apply(x, weight, bias)


def _plain_conv(conv, k, stride):
    return isinstance(conv, torch.nn.Conv2d) and tuple(conv.kernel_size) == (k, k) and tuple(conv.stride) == (stride, stride) and \
        tuple(conv.padding) == (1, 1) and tuple(conv.dilation) == (1, 1) and conv.groups == 1 and \
        getattr(conv, "padding_mode", "zeros") == "zeros"


def _is_up2(m):
    if not isinstance(m, torch.nn.Upsample) or m.mode != "nearest" or m.size is not None or m.scale_factor is None:
        return False
    sf = m.scale_factor
    return all(float(s) == 2.0 for s in (sf if isinstance(sf, (tuple, list)) else (sf, sf)))


def resample_nhwc(module, x):
    """One of the reference's three resampling forms on a channel-last x (B, H, W, Cin) -> channel-last, in x's dtype, with no
    layout copy: a Conv2d(4, 2, 1) (Downsample), a Sequential(nn.Upsample(scale_factor=2, nearest), Conv2d(3, padding 1))
    (Upsample), or a Conv2d(3, padding 1).  Raises RuntimeError, before anything is launched, for any other module, a missing
    bias, unsupported channel counts, an odd H or W in front of a Downsample, a CPU tensor, or inconsistent shapes."""
    fn = "resample_nhwc"
    if isinstance(module, torch.nn.Sequential) and len(module) == 2 and _is_up2(module[0]) and _plain_conv(module[1], 3, 1):
        conv, f = module[1], upsample_fn
    elif _plain_conv(module, 4, 2):
        conv, f = module, downsample_fn
    elif _plain_conv(module, 3, 1):
        conv, f = module, conv3x3_fn
    else:
        raise RuntimeError(f"{fn}: the module must be Conv2d(4, stride 2, padding 1), Sequential(Upsample(scale_factor=2, nearest), "
                           "Conv2d(3, padding 1)) or Conv2d(3, padding 1), with dilation 1, groups 1 and zero padding")
    if conv.bias is None:
        raise RuntimeError(f"{fn}: the convolution must have a bias")
    if not isinstance(x, torch.Tensor):
        raise RuntimeError(f"{fn}: x must be a tensor (got {type(x).__name__})")
    if x.dtype not in (torch.float32,) + HALF:
        raise RuntimeError(f"{fn}: x must be float32 / float16 / bfloat16 (got {x.dtype})")
    if x.dim() != 4 or x.shape[3] != conv.in_channels or min(x.shape) < 1:
        raise RuntimeError(f"{fn}: inconsistent shapes x{tuple(x.shape)} (expected (B, H, W, {conv.in_channels}))")
    return f(x, conv.weight, conv.bias).to(x.dtype)
