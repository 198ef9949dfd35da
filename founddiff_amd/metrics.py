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


INTERVAL_FLOOR = 1 / 3000             # the smallest half-width of a scaled interval: one HU under data.normalize_hu's range
INTERVAL_GRID_MAX = 4096               # grid values per call of fd_interval_hist_f32
_GRIDS = {}                            # (device, the grid's bytes) -> the grid on that device: one upload per distinct grid
_GRIDS_MAX = 16


def _rows(t, B, n):
    """t as it lies in memory, if its slices are dense and a fixed number of floats apart; a dense copy otherwise"""
    t = t.float()
    if not t[0].is_contiguous():
        t = t.contiguous()
    return t, (t.stride(0) if B > 1 else n)


def check_interval_grid(grid):
    """`grid` as a float32 array, or RuntimeError: 1 to 4096 finite, strictly increasing values, the first one >= 0 (host only)"""
    import numpy as np
    g = np.asarray(grid, dtype=np.float32).reshape(-1)
    if not 1 <= g.size <= INTERVAL_GRID_MAX:
        raise RuntimeError(f"interval_hist: the grid must have 1 to {INTERVAL_GRID_MAX} values (got {g.size})")
    if not np.isfinite(g).all():
        raise RuntimeError("interval_hist: the grid must be finite")
    if g[0] < 0:
        raise RuntimeError(f"interval_hist: the grid must start at a value >= 0 (got {float(g[0])})")
    if not (np.diff(g) > 0).all():
        raise RuntimeError("interval_hist: the grid must be strictly increasing (as float32)")
    return g


def _check_floor(what, floor):
    floor = float(floor)
    if not 0 < floor < float("inf"):
        raise RuntimeError(f"{what}: floor must be positive and finite (got {floor})")
    return floor


def interval_hist(center, lo, hi, target, grid, floor=INTERVAL_FLOOR):
    """center, lo, hi, target: fp32 device tensors of one shape (B,...), lo and hi possibly views into one (B,Q,...) tensor of
    quantiles; grid: G ascending scales (checked here, on the host) -> hist (B, G + 1) int64 on the device: hist[b, j] pixels of
    slice b have bin j, the number of grid values strictly below the pixel's score
    max((center - target) / max(center - lo, floor), (target - center) / max(hi - center, floor)), the smallest scale whose
    interval holds the target; bin G: covered by no scale of the grid (a NaN included).  fd_interval_hist_f32."""
    g = check_interval_grid(grid)
    floor = _check_floor("interval_hist", floor)
    if not (center.shape == lo.shape == hi.shape == target.shape) or lo.dim() < 2:
        raise TypeError(f"interval_hist: expected four tensors of one shape (B,...), got {tuple(center.shape)}, {tuple(lo.shape)}, "
                        f"{tuple(hi.shape)} and {tuple(target.shape)}")
    B, G = lo.shape[0], int(g.size)
    n = lo[0].numel()
    key = (str(lo.device), g.tobytes())
    g_dev = _GRIDS.get(key)
    if g_dev is None:
        if len(_GRIDS) >= _GRIDS_MAX:
            _GRIDS.clear()
        g_dev = _GRIDS[key] = torch.from_numpy(g.copy()).to(lo.device)
    (center, cs), (lo, ls), (hi, hs), (target, ts) = (_rows(t, B, n) for t in (center, lo, hi, target))
    nblk = L.lib().fd_interval_hist_nblk(n)
    if nblk <= 0:
        raise L.FoundDiffHipError(f"interval_hist: unsupported slice size {n}")
    ws = torch.empty(B * nblk * (G + 1), device=lo.device, dtype=torch.int32)
    hist = torch.empty(B, G + 1, device=lo.device, dtype=torch.int64)
    stream = C.c_void_p(torch.cuda.current_stream(lo.device).cuda_stream)
    L.call("fd_interval_hist_f32", center.data_ptr(), cs, lo.data_ptr(), ls, hi.data_ptr(), hs, target.data_ptr(), ts,
           g_dev.data_ptr(), G, floor, ws.data_ptr(), hist.data_ptr(), B, n, stream)
    return hist


def interval_scale(center, lo, hi, scale, floor=INTERVAL_FLOOR):
    """center, lo, hi as interval_hist takes them, scale >= 0 -> (lo_out, hi_out of center's shape, width (B,)): the interval with
    both half-widths max(center - lo, floor), max(hi - center, floor) scaled, clamped to [0, 1], and per slice the mean of
    hi_out - lo_out (NaN for a slice with a NaN pixel).  fd_interval_scale_f32."""
    floor, scale = _check_floor("interval_scale", floor), float(scale)
    if not 0 <= scale < float("inf"):
        raise RuntimeError(f"interval_scale: scale must be non-negative and finite (got {scale})")
    if not (center.shape == lo.shape == hi.shape) or lo.dim() < 2:
        raise TypeError(f"interval_scale: expected three tensors of one shape (B,...), got {tuple(center.shape)}, {tuple(lo.shape)} "
                        f"and {tuple(hi.shape)}")
    B = lo.shape[0]
    n = lo[0].numel()
    shape = tuple(center.shape)
    (center, cs), (lo, ls), (hi, hs) = (_rows(t, B, n) for t in (center, lo, hi))
    nblk = L.lib().fd_interval_scale_nblk(n)
    if nblk <= 0:
        raise L.FoundDiffHipError(f"interval_scale: unsupported slice size {n}")
    lo_out = torch.empty(shape, device=lo.device)
    hi_out = torch.empty(shape, device=lo.device)
    ws = torch.empty(B * nblk, device=lo.device)
    width = torch.empty(B, device=lo.device)
    stream = C.c_void_p(torch.cuda.current_stream(lo.device).cuda_stream)
    L.call("fd_interval_scale_f32", center.data_ptr(), cs, lo.data_ptr(), ls, hi.data_ptr(), hs, scale, floor, lo_out.data_ptr(),
           hi_out.data_ptr(), ws.data_ptr(), width.data_ptr(), B, n, stream)
    return lo_out, hi_out, width


def compute_psnr(input, target, max_val=1.0):
    return compute_metrics(input, target)[:, 0].mean()


def compute_ssim(img1, img2):
    return compute_metrics(img1, img2)[:, 1].mean()


def compute_rmse(input, target):
    return compute_metrics(input, target)[:, 2].mean()
