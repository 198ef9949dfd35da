"""The reference's selective-scan extension with its backward, for training:

    out, x, *rest = selective_scan_train.fwd(u, delta, A, B, C, D, delta_bias, delta_softplus, nrows)
    du, ddelta, dA, dB, dC, dD, ddelta_bias = selective_scan_train.bwd(u, delta, A, B, C, D, delta_bias, dout, x,
                                                                       delta_softplus, nrows)

(the calls of src/emamba2.py:154 and 172).  `fwd` IS founddiff_amd.selective_scan_cuda_core.fwd; `bwd` runs
fd_selective_scan_bwd_f32 (csrc/fd_scan_bwd.hip), which recomputes the forward states itself: `x` (the final state
the forward returns) is shape-checked and otherwise unused.  Deterministic: the same inputs give the same bits.

The sampling module selective_scan_cuda_core stays forward-only, so a sampling deployment cannot start differentiating
by accident; a training run binds this module under the extension's name instead:

    import sys, founddiff_amd.selective_scan_train as m
    sys.modules["selective_scan_cuda_core"] = m

`selective_scan_fn(u, delta, A, B, C, D=None, delta_bias=None, delta_softplus=False)` is the same pair as an autograd
function, for code that does not import the reference.
"""
import torch

from . import _lib as L
from ._train import HALF, cast_grads, check_devices, f32, ptr, stream, workspace
from .selective_scan_cuda_core import fwd

__all__ = ["fwd", "bwd", "selective_scan_fn"]


def _chk(name, t, ndim):
    if not isinstance(t, torch.Tensor):
        raise RuntimeError(f"selective_scan_train.bwd: {name} must be a tensor (got {type(t).__name__})")
    if t.dtype not in (torch.float32,) + HALF:
        raise RuntimeError(f"selective_scan_train.bwd: {name} must be float32 / float16 / bfloat16 (got {t.dtype})")
    if t.dim() != ndim:
        raise RuntimeError(f"selective_scan_train.bwd: {name} must be {ndim}-dimensional (got {tuple(t.shape)})")
    if not t.is_cuda:
        raise RuntimeError(f"selective_scan_train.bwd: {name} must live on the GPU (there is no CPU path)")
    return f32(t).contiguous()          # as fwd: the reference's wrapper runs the op in fp32


def bwd(u, delta, A, B, C_, D, delta_bias, dout, x, delta_softplus=False, nrows=1):
    """Gradients of fwd's `out` with respect to its inputs: (du, ddelta, dA, dB, dC, dD, ddelta_bias), fp32, on u's
    device.  dB / dC have B's / C's dimensionality (3-D in, 3-D out); dD / ddelta_bias are None when D / delta_bias are."""
    u, delta, dout = _chk("u", u, 3), _chk("delta", delta, 3), _chk("dout", dout, 3)
    A = _chk("A", A, 2)
    squeeze = B.dim() == 3            # (b, N, L): a single group
    if B.dim() == 3:
        B = B.unsqueeze(1)
    if C_.dim() == 3:
        C_ = C_.unsqueeze(1)
    B, C_ = _chk("B", B, 4), _chk("C", C_, 4)
    b, KD, Ln = u.shape
    K, N = B.shape[1], A.shape[1]
    if (delta.shape != u.shape or dout.shape != u.shape or A.shape[0] != KD or tuple(B.shape) != (b, K, N, Ln)
            or C_.shape != B.shape):
        raise RuntimeError(f"selective_scan_train.bwd: inconsistent shapes u{tuple(u.shape)} delta{tuple(delta.shape)} "
                           f"dout{tuple(dout.shape)} A{tuple(A.shape)} B{tuple(B.shape)} C{tuple(C_.shape)}")
    if x is not None and (not isinstance(x, torch.Tensor) or tuple(x.shape) != (b, KD, N)):
        raise RuntimeError(f"selective_scan_train.bwd: x must be fwd's final state (b, KD, N) = {(b, KD, N)} "
                           f"(got {tuple(x.shape) if isinstance(x, torch.Tensor) else type(x).__name__})")
    if D is not None:
        D = _chk("D", D, 1)
    if delta_bias is not None:
        delta_bias = _chk("delta_bias", delta_bias, 1)
    check_devices("selective_scan_train.bwd", (("u", u), ("delta", delta), ("dout", dout), ("A", A), ("B", B), ("C", C_), ("D", D),
                                               ("delta_bias", delta_bias)))
    with torch.cuda.device(u.device):
        du, ddelta = torch.empty_like(u), torch.empty_like(u)
        dA = torch.empty_like(A)
        dB, dC = torch.empty_like(B), torch.empty_like(C_)
        dD = torch.empty_like(D) if D is not None else None
        dbias = torch.empty_like(delta_bias) if delta_bias is not None else None
        ws = workspace("fd_selective_scan_bwd_ws_floats", u.device, b, KD, K, N, Ln)
        L.call("fd_selective_scan_bwd_f32", ptr(u), ptr(delta), ptr(A), ptr(B), ptr(C_), ptr(D), ptr(delta_bias), ptr(dout),
               int(bool(delta_softplus)), int(nrows), b, KD, K, N, Ln, ptr(du), ptr(ddelta), ptr(dA), ptr(dB), ptr(dC), ptr(dD),
               ptr(dbias), ptr(ws), stream(u.device))
    if squeeze:
        dB, dC = dB.squeeze(1), dC.squeeze(1)
    return du, ddelta, dA, dB, dC, dD, dbias


class _SelectiveScan(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, delta, A, B, C_, D, delta_bias, delta_softplus):
        out, x = fwd(u, delta, A, B, C_, D, delta_bias, delta_softplus, 1)
        ctx.delta_softplus = bool(delta_softplus)
        ctx.dtypes = tuple(t.dtype if t is not None else None for t in (u, delta, A, B, C_, D, delta_bias))
        ctx.save_for_backward(u, delta, A, B, C_, D, delta_bias, x)
        return out

    @staticmethod
    def backward(ctx, dout):
        u, delta, A, B, C_, D, delta_bias, x = ctx.saved_tensors
        grads = bwd(u, delta, A, B, C_, D, delta_bias, dout, x, ctx.delta_softplus, 1)
        return cast_grads(grads, ctx.dtypes) + (None,)


def selective_scan_fn(u, delta, A, B, C, D=None, delta_bias=None, delta_softplus=False):
    """out = the selective scan of fwd, differentiable in u, delta, A, B, C, D and delta_bias."""
    return _SelectiveScan.apply(u, delta, A, B, C, D, delta_bias, delta_softplus)
