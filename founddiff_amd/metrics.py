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


def compute_psnr(input, target, max_val=1.0):
    return compute_metrics(input, target)[:, 0].mean()


def compute_ssim(img1, img2):
    return compute_metrics(img1, img2)[:, 1].mean()


def compute_rmse(input, target):
    return compute_metrics(input, target)[:, 2].mean()
