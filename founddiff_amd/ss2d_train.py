"""The reference's SS2D mixer (src/emamba2.py:404-751) for training: everything between in_proj and out_proj as ONE autograd
function on HIP kernels, channel-last on both passes.

    out = ss2d_core_fn(xz, conv_weight, conv_bias, x_proj_weight, dt_projs_weight, dt_projs_bias, A_logs, Ds,
                       norm_weight, norm_bias, local)
        = LN(scan(SiLU(dwconv3x3(xz[..., :D])))) * SiLU(xz[..., D:]) + local[:, None, None, :]

Forward: fd_dwconv3x3 (reads the x half of xz in place) -> xc, fd_cross_scan_fwd_nhwc_f32 -> x_dbl, y,
fd_ln_silu_gate_fwd_f32 (reads the z half in place) -> out.  Backward: fd_ln_silu_gate_bwd_f32 -> dy and the z half of dxz,
fd_cross_scan_bwd_nhwc_f32 -> dxc, fd_dwconv3x3_silu_bwd_f32 -> the x half of dxz.  Autograd keeps xz (alive anyway as in_proj's
output), xc, x_dbl, y and two floats of LayerNorm statistics per pixel; no permute().contiguous(), chunk or cat copy of an
activation exists on either pass.  Deterministic; a slice's out and dxz do not depend on the batch.  The three GEMMs (in_proj,
out_proj, attn) stay with torch.

Binding for a training run:

    import emamba2, founddiff_amd.ss2d_train as sst
    emamba2.SS2D.forward = sst.ss2d_forward

`SS2D(d_model, d_state, dropout=0.0)` is a module with the reference's parameter names and shapes (its state dict loads with
strict=True) for code that does not import the reference.
"""
import math

import torch

from . import _lib as L
from ._train import cast_grads, check_devices, check_tensors, empty, f32, ptr, stream, workspace

__all__ = ["ss2d_core_fn", "ss2d_forward", "SS2D"]

_N_OK, _R_OK = (4, 8, 16, 32), (2, 4, 8, 16, 32)
_B_MAX = 16383                       # batch x direction is a grid.y of the scan backward: 4 B <= 65535 (cs_shape_ok)
_NAMES = ("xz", "conv_weight", "conv_bias", "x_proj_weight", "dt_projs_weight", "dt_projs_bias", "A_logs", "Ds", "norm_weight",
          "norm_bias", "local")


def _check(xz, conv_weight, conv_bias, x_proj_weight, dt_projs_weight, dt_projs_bias, A_logs, Ds, norm_weight, norm_bias, local):
    """Types, shapes and devices, in that order, before anything is launched (or CUDA initialised)."""
    named = list(zip(_NAMES, (xz, conv_weight, conv_bias, x_proj_weight, dt_projs_weight, dt_projs_bias, A_logs, Ds, norm_weight,
                              norm_bias, local)))
    check_tensors("ss2d_core_fn", named, optional=("conv_bias", "local"))
    shapes = " ".join(f"{n}{tuple(t.shape)}" for n, t in named if t is not None)
    if xz.dim() != 4 or xz.shape[-1] % 2 or dt_projs_weight.dim() != 3 or A_logs.dim() != 2:
        raise RuntimeError(f"ss2d_core_fn: inconsistent shapes {shapes} (xz is (B, H, W, 2 d_inner))")
    B, H, W, D2 = xz.shape
    D = D2 // 2
    K, Dw, R = dt_projs_weight.shape
    KD, N = A_logs.shape
    ok = (K == 4 and Dw == D and KD == 4 * D and tuple(x_proj_weight.shape) == (4, R + 2 * N, D)
          and tuple(dt_projs_bias.shape) in ((4, D), (4 * D,)) and tuple(Ds.shape) == (4 * D,)
          and tuple(conv_weight.shape) == (D, 1, 3, 3) and (conv_bias is None or tuple(conv_bias.shape) == (D,))
          and tuple(norm_weight.shape) == (D,) and tuple(norm_bias.shape) == (D,)
          and (local is None or tuple(local.shape) in ((B, D), (B, 1, D))))
    if not ok:
        raise RuntimeError(f"ss2d_core_fn: inconsistent shapes {shapes} (4 directions, d_inner = xz.shape[-1] / 2, conv_weight "
                           "(d_inner, 1, 3, 3), local (B, d_inner) or (B, 1, d_inner))")
    if D % 64 or D > 1024 or N not in _N_OK or R not in _R_OK or not 1 <= B <= _B_MAX or H < 1 or W < 1:
        raise RuntimeError(f"ss2d_core_fn: unsupported shape d_inner={D} (multiple of 64, at most 1024), d_state={N} (one of "
                           f"{_N_OK}), dt_rank={R} (one of {_R_OK}), image {H}x{W}, batch {B} (at most {_B_MAX})")
    check_devices("ss2d_core_fn", named)
    return B, H, W, D, N, R


class _SS2DCore(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xz, conv_weight, conv_bias, x_proj_weight, dt_projs_weight, dt_projs_bias, A_logs, Ds, norm_weight, norm_bias,
                local, eps):
        args = (xz, conv_weight, conv_bias, x_proj_weight, dt_projs_weight, dt_projs_bias, A_logs, Ds, norm_weight, norm_bias, local)
        B, H, W, D, N, R = _check(*args)
        ctx.dtypes = tuple(None if t is None else t.dtype for t in args)
        ctx.shapes = (dt_projs_bias.shape, None if local is None else local.shape)
        xz, cw, cb, xw, dtw, dtb, Al, Dv, gw, gb, loc = (None if t is None else f32(t).contiguous() for t in args)
        w9 = cw.reshape(D, 9).t().contiguous()               # [9][D] tap-major, as fd_dwconv3x3 takes it
        A = -torch.exp(Al)
        loc2 = None if loc is None else loc.reshape(B, D)
        dev = xz.device
        L2 = ((H + 1) // 2) * ((W + 1) // 2)
        with torch.cuda.device(dev):
            new = empty(dev)
            xc, y, out = new(B, H, W, D), new(B, H, W, D), new(B, H, W, D)
            xdbl, stats = new(4, B, L2, R + 2 * N), new(B, H, W, 2)
            ws = workspace("fd_scan_ws_floats", dev, B, H, W, D, N)
            L.call("fd_dwconv3x3", L.FD_F32, ptr(xz), 2 * D, 0, ptr(w9), ptr(cb), 1, ptr(xc), D, 0, B, H, W, D, stream(dev))
            L.call("fd_cross_scan_fwd_nhwc_f32", ptr(xc), ptr(xw), ptr(dtw), ptr(dtb), ptr(A), ptr(Dv), ptr(xdbl), ptr(y), ptr(ws),
                   B, H, W, D, N, R, stream(dev))
            L.call("fd_ln_silu_gate_fwd_f32", ptr(y), ptr(gw), ptr(gb), float(eps), ptr(xz), 2 * D, D, ptr(loc2), D, ptr(out),
                   ptr(stats), B, H * W, D, stream(dev))
        ctx.dims = (B, H, W, D, N, R)
        ctx.has = (cb is not None, loc is not None)
        ctx.save_for_backward(xz, xc, xdbl, y, stats, w9, cb, xw, dtw, dtb, A, Dv, gw, gb)
        return out

    @staticmethod
    def backward(ctx, dout):
        xz, xc, xdbl, y, stats, w9, cb, xw, dtw, dtb, A, Dv, gw, gb = ctx.saved_tensors
        B, H, W, D, N, R = ctx.dims
        has_bias, has_local = ctx.has
        if tuple(dout.shape) != (B, H, W, D):
            raise RuntimeError(f"ss2d_core_fn: the gradient of out must be {(B, H, W, D)} (got {tuple(dout.shape)})")
        dout = f32(dout).contiguous()
        dev = xz.device
        with torch.cuda.device(dev):
            new = empty(dev)
            dxz, dy = new(B, H, W, 2 * D), new(B, H, W, D)
            dgw, dgb = new(D), new(D)
            dloc = new(B, D) if has_local else None
            ws = workspace("fd_ln_silu_gate_bwd_ws_floats", dev, B, H * W, D)
            L.call("fd_ln_silu_gate_bwd_f32", ptr(dout), ptr(y), ptr(stats), ptr(gw), ptr(gb), ptr(xz), 2 * D, D, ptr(dy), ptr(dxz),
                   2 * D, D, ptr(dgw), ptr(dgb), ptr(dloc), ptr(ws), B, H * W, D, stream(dev))
            dxc = new(B, H, W, D)
            dxw, ddtw, ddtb, dA, dDs = torch.empty_like(xw), torch.empty_like(dtw), new(4 * D), torch.empty_like(A), torch.empty_like(Dv)
            ws = workspace("fd_cross_scan_bwd_ws_floats", dev, B, H, W, D, N, R)
            L.call("fd_cross_scan_bwd_nhwc_f32", ptr(xc), ptr(xdbl), ptr(xw), ptr(dtw), ptr(dtb), ptr(A), ptr(Dv), ptr(dy), ptr(dxc),
                   ptr(dxw), ptr(ddtw), ptr(ddtb), ptr(dA), ptr(dDs), ptr(ws), B, H, W, D, N, R, stream(dev))
            del dy
            dw9, dcb = new(9, D), (new(D) if has_bias else None)
            ws = workspace("fd_dwconv3x3_silu_bwd_ws_floats", dev, B, H, W, D)
            L.call("fd_dwconv3x3_silu_bwd_f32", ptr(xz), 2 * D, 0, ptr(w9), ptr(cb), ptr(dxc), ptr(dxz), 2 * D, 0, ptr(dw9), ptr(dcb),
                   ptr(ws), B, H, W, D, stream(dev))
            del dxc, ws
        bias_shape, local_shape = ctx.shapes
        grads = (dxz, dw9.t().reshape(D, 1, 3, 3), dcb, dxw, ddtw, ddtb.view(bias_shape), dA * A, dDs, dgw, dgb,
                 None if dloc is None else dloc.view(local_shape))       # A = -exp(A_logs): dA_logs = dA * A
        return cast_grads(grads, ctx.dtypes) + (None,)


def ss2d_core_fn(xz, conv_weight, conv_bias, x_proj_weight, dt_projs_weight, dt_projs_bias, A_logs, Ds, norm_weight, norm_bias,
                 local=None, eps=1e-5):
    """(B, H, W, d_inner) fp32, differentiable in every tensor argument.  xz (B, H, W, 2 d_inner): in_proj's output;
    conv_weight (d_inner, 1, 3, 3), conv_bias (d_inner) or None; x_proj_weight (4, R + 2N, d_inner); dt_projs_weight
    (4, d_inner, R); dt_projs_bias (4, d_inner); A_logs (4 d_inner, N); Ds (4 d_inner); norm_weight, norm_bias (d_inner): out_norm;
    local (B, d_inner) or (B, 1, d_inner) or None.  16-bit tensors are up-cast; their gradients come back in their dtypes."""
    _check(xz, conv_weight, conv_bias, x_proj_weight, dt_projs_weight, dt_projs_bias, A_logs, Ds, norm_weight, norm_bias, local)
    return _SS2DCore.apply(xz, conv_weight, conv_bias, x_proj_weight, dt_projs_weight, dt_projs_bias, A_logs, Ds, norm_weight,
                           norm_bias, local, eps)


def ss2d_forward(self, x, c, **kwargs):
    """SS2D.forward (src/emamba2.py:713-751): x (B, H, W, d_model), c (B, 1, 256) -> (B, H, W, d_model) in x's dtype.  Reads the
    reference's attribute names.  Raises RuntimeError, before anything is launched, for what the shipped constructor never
    builds: d_conv != 3, ssm_low_rank, an out_norm that is not a LayerNorm, step_size != 2."""
    if getattr(self, "d_conv", 3) != 3:
        raise RuntimeError(f"ss2d_forward: d_conv={self.d_conv} is not supported (only 3, the shipped value)")
    if getattr(self, "ssm_low_rank", False):
        raise RuntimeError("ss2d_forward: ssm_low_rank is not supported (the shipped SS2D has d_inner = d_expand)")
    if getattr(self, "step_size", 2) != 2:
        raise RuntimeError(f"ss2d_forward: step_size={self.step_size} is not supported (only 2, the shipped value)")
    norm = self.out_norm
    if not isinstance(norm, torch.nn.LayerNorm) or norm.weight is None or norm.bias is None:
        raise RuntimeError(f"ss2d_forward: out_norm must be an affine LayerNorm (got {type(norm).__name__})")
    conv = self.conv2d
    if tuple(conv.kernel_size) != (3, 3) or tuple(conv.padding) != (1, 1) or conv.groups != conv.in_channels or \
            tuple(conv.stride) != (1, 1) or tuple(conv.dilation) != (1, 1):
        raise RuntimeError("ss2d_forward: conv2d must be a depthwise 3x3 convolution with padding 1")
    for name, t in (("x", x), ("c", c)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"ss2d_forward: {name} must be a tensor on the GPU (there is no CPU path)")
    if x.dim() != 4 or x.shape[-1] != self.in_proj.in_features:
        raise RuntimeError(f"ss2d_forward: inconsistent shapes x{tuple(x.shape)} (expected (B, H, W, {self.in_proj.in_features}))")
    local = self.attn(c)
    xz = self.in_proj(x)
    y = ss2d_core_fn(xz, conv.weight, conv.bias, self.x_proj_weight, self.dt_projs_weight, self.dt_projs_bias, self.A_logs, self.Ds,
                     norm.weight, norm.bias, local, norm.eps)
    return self.dropout(self.out_proj(y.to(xz.dtype)))


class SS2D(torch.nn.Module):
    """The reference's SS2D as its shipped constructor builds it: ssm_ratio 2 (d_inner = 2 d_model), dt_rank = ceil(d_model / 16),
    K = 4 directions, depthwise 3 x 3 conv with bias, LayerNorm out_norm, bias-free in_proj / out_proj, attn = Linear(256,
    d_inner, bias=False) + SiLU.  Parameter names and shapes are the reference's.  Initialisation: x_proj ~ d_inner^-0.5,
    dt_proj ~ dt_rank^-0.5, the dt bias the softplus inverse of a log-uniform dt in [1e-3, 1e-1], A_logs = log(1 .. N), Ds = 1;
    the torch layers keep torch's defaults."""

    def __init__(self, d_model, d_state, dropout=0.0):
        super().__init__()
        nn = torch.nn
        D = 2 * d_model
        self.d_model, self.d_state, self.d_conv, self.step_size, self.ssm_low_rank = d_model, d_state, 3, 2, False
        self.dt_rank = R = math.ceil(d_model / 16)
        self.in_proj = nn.Linear(d_model, 2 * D, bias=False)
        self.conv2d = nn.Conv2d(D, D, 3, padding=1, groups=D, bias=True)
        self.x_proj_weight = nn.Parameter((torch.rand(4, R + 2 * d_state, D) * 2 - 1) * D ** -0.5)
        self.dt_projs_weight = nn.Parameter((torch.rand(4, D, R) * 2 - 1) * R ** -0.5)
        dt = torch.exp(torch.rand(4, D) * (math.log(0.1) - math.log(1e-3)) + math.log(1e-3)).clamp(min=1e-4)
        self.dt_projs_bias = nn.Parameter(dt + torch.log(-torch.expm1(-dt)))
        self.A_logs = nn.Parameter(torch.log(torch.arange(1, d_state + 1, dtype=torch.float32))[None].repeat(4 * D, 1))
        self.Ds = nn.Parameter(torch.ones(4 * D))
        self.out_norm = nn.LayerNorm(D)
        self.out_proj = nn.Linear(D, d_model, bias=False)
        self.dropout = nn.Dropout(dropout) if dropout > 0.0 else nn.Identity()
        self.attn = nn.Sequential(nn.Linear(256, D, bias=False), nn.SiLU())

    forward = ss2d_forward
