"""The reference's cross_selective_scan (src/emamba2.py:295-367) for training, on the fused dataflow of the sampling engine:

    y = cross_selective_scan(x, x_proj_weight, None, dt_projs_weight, dt_projs_bias, A_logs, Ds, out_norm,
                             nrows=nrows, delta_softplus=True, step_size=2)

(forward_corev2's call, src/emamba2.py:704-708).  The forward is fd_cross_scan_fwd_f32 (NCHW -> NHWC, the x_proj gather as one
fd_conv2d launch, fd_selective_scan in fp32), the backward fd_cross_scan_bwd_f32 (csrc/fd_cross_scan_bwd.hip).  Neither
EfficientScan's gathered copy, nor delta, nor EfficientMerge's scatter ever exists: autograd keeps xc (the NHWC input) and
x_dbl (the x_proj rows) and nothing else of the op.  Deterministic, and a slice's y and dx do not depend on the batch.

Binding for a training run; forward_corev2 looks the name up at call time:

    import emamba2, founddiff_amd.cross_scan_train as cst
    emamba2.cross_selective_scan = cst.cross_selective_scan

`cross_scan_fn(x, x_proj_weight, dt_projs_weight, dt_projs_bias, A_logs, Ds)` is the autograd function underneath: y before
out_norm as (B, H, W, d_inner) fp32, for code that does not import the reference.
"""
import torch

from . import _lib as L
from ._train import HALF, cast_grads, check_devices, empty, f32, ptr, stream, workspace

__all__ = ["cross_selective_scan", "cross_scan_fn"]

_N_OK, _R_OK = (4, 8, 16, 32), (2, 4, 8, 16, 32)
_B_MAX = 16383                       # batch x direction is a grid.y of the backward: 4 B <= 65535 (cs_shape_ok)


def _f32(name, t):
    """a tensor _check (or autograd) let through, as the kernels take it: the op runs in fp32, as selective_scan_train"""
    if t.dtype not in (torch.float32,) + HALF:
        raise RuntimeError(f"cross_selective_scan: {name} must be float32 / float16 / bfloat16 (got {t.dtype})")
    return f32(t).contiguous()


def _check(x, x_proj_weight, dt_projs_weight, dt_projs_bias, A_logs, Ds):
    """Shapes and devices, before anything is launched (or CUDA initialised)."""
    named = (("x", x), ("x_proj_weight", x_proj_weight), ("dt_projs_weight", dt_projs_weight),
             ("dt_projs_bias", dt_projs_bias), ("A_logs", A_logs), ("Ds", Ds))
    for name, t in named:
        if not isinstance(t, torch.Tensor):
            raise RuntimeError(f"cross_selective_scan: {name} must be a tensor (got {type(t).__name__})")
        if not t.is_cuda:
            raise RuntimeError(f"cross_selective_scan: {name} must live on the GPU (there is no CPU path)")
    if x.dim() != 4 or dt_projs_weight.dim() != 3 or x_proj_weight.dim() != 3 or A_logs.dim() != 2:
        raise RuntimeError(f"cross_selective_scan: inconsistent shapes x{tuple(x.shape)} x_proj_weight{tuple(x_proj_weight.shape)} "
                           f"dt_projs_weight{tuple(dt_projs_weight.shape)} A_logs{tuple(A_logs.shape)}")
    B, D, H, W = x.shape
    K, Dw, R = dt_projs_weight.shape
    KD, N = A_logs.shape
    ok = (K == 4 and Dw == D and KD == 4 * D and tuple(x_proj_weight.shape) == (4, R + 2 * N, D)
          and dt_projs_bias.numel() == 4 * D and tuple(dt_projs_bias.shape) in ((4, D), (4 * D,))
          and tuple(Ds.shape) == (4 * D,))
    if not ok:
        raise RuntimeError(f"cross_selective_scan: inconsistent shapes x{tuple(x.shape)} x_proj_weight{tuple(x_proj_weight.shape)} "
                           f"dt_projs_weight{tuple(dt_projs_weight.shape)} dt_projs_bias{tuple(dt_projs_bias.shape)} "
                           f"A_logs{tuple(A_logs.shape)} Ds{tuple(Ds.shape)} (4 directions, d_inner = x.shape[1])")
    if D % 64 or N not in _N_OK or R not in _R_OK or not 1 <= B <= _B_MAX or H < 1 or W < 1:
        raise RuntimeError(f"cross_selective_scan: unsupported shape d_inner={D} (multiple of 64), d_state={N} (one of {_N_OK}), "
                           f"dt_rank={R} (one of {_R_OK}), image {H}x{W}, batch {B} (at most {_B_MAX})")
    check_devices("cross_selective_scan", named)
    return B, D, H, W, N, R


class _CrossScan(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, x_proj_weight, dt_projs_weight, dt_projs_bias, A_logs, Ds):
        B, D, H, W, N, R = _check(x, x_proj_weight, dt_projs_weight, dt_projs_bias, A_logs, Ds)
        ctx.dtypes = tuple(t.dtype for t in (x, x_proj_weight, dt_projs_weight, dt_projs_bias, A_logs, Ds))
        ctx.bias_shape = dt_projs_bias.shape
        xw, dtw, dtb, Al, Dv = (_f32(n, t) for n, t in (("x_proj_weight", x_proj_weight), ("dt_projs_weight", dt_projs_weight),
                                                          ("dt_projs_bias", dt_projs_bias), ("A_logs", A_logs), ("Ds", Ds)))
        x = _f32("x", x)
        A = -torch.exp(Al)
        L2 = ((H + 1) // 2) * ((W + 1) // 2)
        dev = x.device
        with torch.cuda.device(dev):
            new = empty(dev)
            xc, xdbl, y = new(B, H, W, D), new(4, B, L2, R + 2 * N), new(B, H, W, D)
            ws = workspace("fd_scan_ws_floats", dev, B, H, W, D, N)
            L.call("fd_cross_scan_fwd_f32", ptr(x), ptr(xw), ptr(dtw), ptr(dtb), ptr(A), ptr(Dv), ptr(xc), ptr(xdbl), ptr(y), ptr(ws),
                   B, H, W, D, N, R, stream(dev))
        ctx.dims = (B, D, H, W, N, R)
        ctx.save_for_backward(xc, xdbl, xw, dtw, dtb, A, Dv)
        return y

    @staticmethod
    def backward(ctx, dy):
        xc, xdbl, xw, dtw, dtb, A, Dv = ctx.saved_tensors
        B, D, H, W, N, R = ctx.dims
        dy = _f32("dy", dy)
        if tuple(dy.shape) != (B, H, W, D):
            raise RuntimeError(f"cross_selective_scan: the gradient of y must be {(B, H, W, D)} (got {tuple(dy.shape)})")
        dev = xc.device
        with torch.cuda.device(dev):
            dx = torch.empty(B, D, H, W, device=dev, dtype=torch.float32)
            dxw, ddtw, ddtb = torch.empty_like(xw), torch.empty_like(dtw), torch.empty(4 * D, device=dev, dtype=torch.float32)
            dA, dDs = torch.empty_like(A), torch.empty_like(Dv)
            ws = workspace("fd_cross_scan_bwd_ws_floats", dev, B, H, W, D, N, R)
            L.call("fd_cross_scan_bwd_f32", ptr(xc), ptr(xdbl), ptr(xw), ptr(dtw), ptr(dtb), ptr(A), ptr(Dv), ptr(dy), ptr(dx),
                   ptr(dxw), ptr(ddtw), ptr(ddtb), ptr(dA), ptr(dDs), ptr(ws), B, H, W, D, N, R, stream(dev))
        dA_logs = dA * A                                     # A = -exp(A_logs): dA_logs = dA * dA/dA_logs = dA * A
        grads = (dx, dxw, ddtw, ddtb.view(ctx.bias_shape), dA_logs, dDs)
        return cast_grads(grads, ctx.dtypes)


def cross_scan_fn(x, x_proj_weight, dt_projs_weight, dt_projs_bias, A_logs, Ds):
    """y before out_norm, (B, H, W, d_inner) fp32, differentiable in every argument.  x (B, d_inner, H, W); x_proj_weight
    (4, R + 2N, d_inner); dt_projs_weight (4, d_inner, R); dt_projs_bias (4, d_inner); A_logs (4 d_inner, N); Ds (4 d_inner)."""
    return _CrossScan.apply(x, x_proj_weight, dt_projs_weight, dt_projs_bias, A_logs, Ds)


def cross_selective_scan(x, x_proj_weight=None, x_proj_bias=None, dt_projs_weight=None, dt_projs_bias=None,
                         A_logs=None, Ds=None, out_norm=None, nrows=-1, delta_softplus=True, to_dtype=True, step_size=2):
    """src/emamba2.py:295-367 with the same signature and result: out_norm(y).view(B, H, W, d_inner), cast back to x.dtype when
    to_dtype.  `nrows` is accepted and ignored (the reference's own backward passes 1).  Raises before any launch for what
    SS2D never passes: an x_proj bias, step_size != 2, delta_softplus=False, CPU tensors, inconsistent shapes."""
    if x_proj_bias is not None:
        raise RuntimeError("cross_selective_scan: x_proj_bias is not supported (SS2D passes None, src/emamba2.py:705)")
    if step_size != 2:
        raise RuntimeError(f"cross_selective_scan: step_size={step_size} is not supported (only 2, SS2D's value)")
    if not delta_softplus:
        raise RuntimeError("cross_selective_scan: delta_softplus=False is not supported (SS2D passes True)")
    _check(x, x_proj_weight, dt_projs_weight, dt_projs_bias, A_logs, Ds)
    B, D, H, W = x.shape
    y = cross_scan_fn(x, x_proj_weight, dt_projs_weight, dt_projs_bias, A_logs, Ds)
    if out_norm is not None:
        y = out_norm(y)
    y = y.view(B, H, W, -1)
    return y.to(x.dtype) if to_dtype else y
