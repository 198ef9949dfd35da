"""What the training bindings (*_train.py) share: the argument checks that fire before anything is launched, the pointer / stream /
workspace expressions of a library call, the casts around one, and fd_conv2d in its exact-fp32 form."""
import ctypes as C

import torch

from . import _lib as L

HALF = (torch.float16, torch.bfloat16)


def f32(t):
    return t.float() if t.dtype in HALF else t


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def workspace(name, dev, *args):
    n = int(getattr(L.lib(), name)(*args))
    return torch.empty(max(n, 4), device=dev, dtype=torch.float32)      # the caching allocator's blocks are 512-byte aligned


def empty(dev):
    return lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)


def check_tensors(fn, named, optional=()):
    """Types and dtypes.  The callers test shapes next and devices (check_devices) last."""
    for name, t in named:
        if t is None and name in optional:
            continue
        if not isinstance(t, torch.Tensor):
            raise RuntimeError(f"{fn}: {name} must be a tensor (got {type(t).__name__})")
        if t.dtype not in (torch.float32,) + HALF:
            raise RuntimeError(f"{fn}: {name} must be float32 / float16 / bfloat16 (got {t.dtype})")


def check_devices(fn, named):
    first = named[0][1]
    for name, t in named:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError(f"{fn}: {name} must live on the GPU (there is no CPU path)")
        if t.device != first.device:
            raise RuntimeError(f"{fn}: {name} lives on {t.device}, {named[0][0]} on {first.device}")


def grad_out(fn, dout, dims):
    if tuple(dout.shape) != tuple(dims):
        raise RuntimeError(f"{fn}: the gradient of the result must be {tuple(dims)} (got {tuple(dout.shape)})")
    return f32(dout).contiguous()


def cast_grads(grads, dtypes):
    return tuple(None if g is None else (g.to(dt) if g.dtype != dt else g) for g, dt in zip(grads, dtypes))


def strided(t, C3):
    """(tensor, ld, off) for the kernels: t itself if it is a channel slice of a dense (B, H, W, ld) tensor, else a dense copy"""
    B, H, W, _ = t.shape
    ld = t.stride(2)
    if t.stride() == (H * W * ld, W * ld, ld, 1) and ld >= C3 and ld % 4 == 0:
        off = t.storage_offset() % ld
        if off % 4 == 0 and off + C3 <= ld and (t.data_ptr() - 4 * off) % 16 == 0:
            return t, ld, off
    return t.contiguous(), C3, 0


def conv2d_f32(x, ld, off, cin, wk, bias, cout, dims, k=3, stride=1, stats=None):
    """fd_conv2d, exact fp32, k x k / stride / padding 1: x channels [off, off + cin) of (B, H, W, ld); wk [cout][k k cin], K
    order (kh, kw, c); stats: the GroupNorm partial sums of the epilogue, or None"""
    B, H, W = dims
    OH, OW = (H + 2 - k) // stride + 1, (W + 2 - k) // stride + 1
    out = torch.empty(B, OH, OW, cout, device=x.device, dtype=torch.float32)
    p = L.ConvParams()
    p.dtype, p.out_f32 = L.FD_F32, 0
    p.in0, p.c0, p.ld0, p.off0 = x.data_ptr() - 4 * off, cin, ld, off
    p.B, p.H, p.W, p.OH, p.OW = B, H, W, OH, OW
    p.KH, p.KW, p.stride, p.pad_h, p.pad_w, p.ndir = k, k, stride, 1, 1, 1
    p.weight, p.bias = wk.data_ptr(), (None if bias is None else bias.data_ptr())
    p.Cout, p.out, p.ldo, p.offo = cout, out.data_ptr(), cout, 0
    p.epilogue, p.ld_res, p.gn_groups = L.EPI_NONE, cout, 1
    p.stats_partial = None if stats is None else stats.data_ptr()
    p.f32_split = 0
    L.call("fd_conv2d", C.byref(p), stream(x.device))
    return out
