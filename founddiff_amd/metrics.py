"""PSNR / SSIM / RMSE of Trainer.test on the device (reference: src/util.py:188-236)."""
import ctypes as C

import torch

from . import _lib as L


def compute_metrics(pred, target):
    """pred, target: (B,1,H,W) or (B,H,W) fp32 device tensors in [0,1] -> (B,3) = PSNR, SSIM, RMSE."""
    pred = pred.contiguous().float()
    target = target.contiguous().float()
    if pred.shape != target.shape:
        raise TypeError(f"Expected tensors of equal shapes, but got {pred.shape} and {target.shape}")
    H, W = pred.shape[-2:]
    B = pred.numel() // (H * W)
    nblk = L.lib().fd_metrics_nblk(H, W)
    ws = torch.empty(B, nblk, 2, device=pred.device)
    out = torch.empty(B, 3, device=pred.device)
    stream = C.c_void_p(torch.cuda.current_stream(pred.device).cuda_stream)
    L.call("fd_metrics", pred.data_ptr(), target.data_ptr(), B, H, W, ws.data_ptr(), out.data_ptr(), stream)
    return out


def ensemble_stats(samples):
    """samples (B,K,...) fp32 device tensor, K realisations per slice -> (mean, std) of shape (B,...) and spread (B,): the per-pixel
    mean and two-pass sample standard deviation over k (0 for K = 1) and sqrt(mean over pixels of std^2), fd_ensemble_stats_f32."""
    samples = samples.contiguous().float()
    B, K = samples.shape[:2]
    n = samples[0, 0].numel()
    nblk = L.lib().fd_ensemble_nblk(n)
    if nblk <= 0:
        raise L.FoundDiffHipError(f"ensemble_stats: unsupported slice size {n}")
    mean = torch.empty((B,) + tuple(samples.shape[2:]), device=samples.device)
    std = torch.empty_like(mean)
    ws = torch.empty(B * nblk, device=samples.device)
    spread = torch.empty(B, device=samples.device)
    stream = C.c_void_p(torch.cuda.current_stream(samples.device).cuda_stream)
    L.call("fd_ensemble_stats_f32", samples.data_ptr(), mean.data_ptr(), std.data_ptr(), ws.data_ptr(), spread.data_ptr(), B, K, n,
           stream)
    return mean, std, spread


def ensemble_quantiles(samples, levels):
    """samples (B,K,...) fp32 device tensor, K realisations per slice -> (B,Q,...): per pixel the Q = len(levels) quantiles over k under
    the `linear` rule (ensemble.quantile_table), fd_ensemble_order_f32.  A level that falls on a sample (minimum, maximum, the median
    of an odd K) is that sample bit for bit; a pixel with a NaN among its K values is NaN at every level."""
    from .ensemble import quantile_table
    samples = samples.contiguous().float()
    B, K = samples.shape[:2]
    lo, hi, frac = quantile_table(levels, K)
    Q = len(lo)
    n = samples[0, 0].numel()
    out = torch.empty((B, Q) + tuple(samples.shape[2:]), device=samples.device)
    stream = C.c_void_p(torch.cuda.current_stream(samples.device).cuda_stream)
    L.call("fd_ensemble_order_f32", samples.data_ptr(), out.data_ptr(), (L.i32 * Q)(*lo.tolist()), (L.i32 * Q)(*hi.tolist()),
           (L.f32 * Q)(*frac.tolist()), B, K, Q, n, stream)
    return out


def interval_coverage(lo, hi, target):
    """lo, hi, target: fp32 device tensors of one shape (B,...), lo and hi possibly views into one (B,Q,...) tensor of quantiles ->
    (count (B,) int64 on the device, fraction (B,) float64 on the host): the pixels of a slice with lo <= target <= hi, counted
    exactly (a NaN is outside), and that count over the slice's pixels.  fd_ensemble_coverage_f32."""
    if not (lo.shape == hi.shape == target.shape) or lo.dim() < 2:
        raise TypeError(f"interval_coverage: expected three tensors of one shape (B,...), got {tuple(lo.shape)}, {tuple(hi.shape)} "
                        f"and {tuple(target.shape)}")
    B = lo.shape[0]
    n = lo[0].numel()

    def rows(t):
        """t as it lies in memory, if its slices are dense and a fixed number of floats apart; a dense copy otherwise"""
        t = t.float()
        if not t[0].is_contiguous():
            t = t.contiguous()
        return t, (t.stride(0) if B > 1 else n)
    (lo, ls), (hi, hs), (target, ts) = rows(lo), rows(hi), rows(target)
    nblk = L.lib().fd_ensemble_coverage_nblk(n)
    if nblk <= 0:
        raise L.FoundDiffHipError(f"interval_coverage: unsupported slice size {n}")
    ws = torch.empty(B * nblk, device=lo.device, dtype=torch.int32)
    count = torch.empty(B, device=lo.device, dtype=torch.int64)
    stream = C.c_void_p(torch.cuda.current_stream(lo.device).cuda_stream)
    L.call("fd_ensemble_coverage_f32", lo.data_ptr(), ls, hi.data_ptr(), hs, target.data_ptr(), ts, ws.data_ptr(), count.data_ptr(), B,
           n, stream)
    return count, count.cpu().numpy().astype("float64") / n


def compute_psnr(input, target, max_val=1.0):
    return compute_metrics(input, target)[:, 0].mean()


def compute_ssim(img1, img2):
    return compute_metrics(img1, img2)[:, 1].mean()


def compute_rmse(input, target):
    return compute_metrics(input, target)[:, 2].mean()
