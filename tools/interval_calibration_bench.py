"""Calibrated intervals (metrics.interval_hist / interval_scale, csrc/fd_interval.hip; Trainer.calibrate_intervals): what the score
histogram and the scaled maps cost.  Everything is reported, nothing is gated.  --size x --size slices, one JSON line per leg:

  leg 1  fd_interval_hist_f32 alone on --slices slices: "phantom" (synth.ct_phantom with K = 8 multiplicative-noise replicas, their
         mean and 0.05 / 0.95 levels: the air is exactly 0 in every map, so a third of the pixels share bin 0) and "uniform" (scores
         spread evenly over the grid), at G = 1025 (ensemble.interval_grid()); the uniform leg twice more, which is the run-to-run
         spread the phantom leg is read against; the phantom leg again at G = 1 and G = 4096.  Each is alternated in this process
         with the torch composition it replaces (the score in torch, torch.bucketize, torch.bincount per slice).  Milliseconds from
         device events around --inner back-to-back calls, the median of --reps rounds after two untimed ones; the kernel's bytes
         (four maps read), those bytes per second and over 6.3 TB/s; torch's time over the kernel's; torch's peak extra device
         memory; whether the two count the same.
  leg 2  fd_interval_scale_f32 the same way (three maps read, two written) against clamp / mul / sub / mean in torch.
  leg 3  Trainer.calibrate_intervals on --cal-slices slices x K = 8 at 2 DDIM steps (bf16, the shipped architecture with synthetic
         weights) against the same sample_ensemble calls without the scoring: wall milliseconds to the closing synchronisation,
         alternated, the median of --reps rounds after one untimed round.

    python tools/interval_calibration_bench.py [--size 512] [--slices 8] [--reps 3] [--inner 20] [--cal-slices 16] [--out FILE]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PREFIX = "model.unet0."
HBM_BPS = 6.3e12
LEVELS = (0.05, 0.95)
FLOOR = 1 / 3000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--slices", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--cal-slices", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "interval_calibration_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/interval_calibration_bench.py measures on the GPU: none is visible")
    dev = torch.device("cuda:0")
    from founddiff_amd import arch, synth
    from founddiff_amd.DADiff import ResidualDiffusion, Trainer, UnetRes, load_weights
    from founddiff_amd.data import SyntheticCTDataset
    from founddiff_amd.ensemble import interval_grid
    from founddiff_amd.metrics import ensemble_quantiles, interval_hist, interval_scale
    S, B = a.size, a.slices
    npix = S * S
    rows = []
    med = lambda v: sorted(v)[len(v) // 2]

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.inner):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.inner

    def alternate(legs):
        ts = {tag: [] for tag, _ in legs}
        for it in range(2 + a.reps):
            for tag, fn in legs:
                t = timed(fn)
                if it >= 2:
                    ts[tag].append(t)
        return ts

    def peak_extra(fn, out_bytes):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        return out, torch.cuda.max_memory_allocated() - base - out_bytes

    # the inputs
    nd = torch.from_numpy(synth.ct_phantom(B, S, seed=10)[0]).to(dev).reshape(B, 1, npix)
    g = torch.Generator(device=dev).manual_seed(1)
    samples = (nd * (1 + 0.02 * torch.randn(B, 8, npix, device=dev, generator=g))).clamp_(0, 1)     # air stays 0 in every replica
    q = ensemble_quantiles(samples, LEVELS)
    phantom = (samples.mean(1).contiguous(), q[:, 0].contiguous(), q[:, 1].contiguous(), nd[:, 0].contiguous())
    half = torch.full((B, npix), 0.5, device=dev)
    uniform = (half, half - 0.125, half + 0.25, half + 0.25 * 16 * torch.rand(B, npix, device=dev, generator=g))
    air = float((phantom[3] == 0).float().mean())
    del samples, q

    def torch_hist(m, l, u, y, grid_dev):
        G = grid_dev.numel()
        s = torch.maximum((m - y) / (m - l).clamp_min(FLOOR), (y - m) / (u - m).clamp_min(FLOOR))
        b = torch.where(torch.isnan(s), G, torch.bucketize(s, grid_dev))          # grid[b - 1] < s <= grid[b]
        return torch.stack([torch.bincount(b[i], minlength=G + 1) for i in range(B)])

    def torch_scale(m, l, u, scale):
        lo = (m - scale * (m - l).clamp_min(FLOOR)).clamp_(0, 1)
        hi = (m + scale * (u - m).clamp_min(FLOOR)).clamp_(0, 1)
        return lo, hi, (hi - lo).mean(1)

    # leg 1: the histogram kernel against bucketize + bincount
    grids = {1: np.array([1.0], np.float32), 1025: interval_grid(), 4096: np.linspace(0, 16, 4096).astype(np.float32)}
    for data, maps, G, rep in (("phantom", phantom, 1025, 0), ("uniform", uniform, 1025, 0), ("uniform", uniform, 1025, 1),
                               ("uniform", uniform, 1025, 2), ("phantom", phantom, 1, 0), ("phantom", phantom, 4096, 0),
                               ("uniform", uniform, 4096, 0)):
        grid = grids[G]
        grid_dev = torch.from_numpy(grid).to(dev)
        ts = alternate((("hip", lambda: interval_hist(*maps, grid)), ("torch", lambda: torch_hist(*maps, grid_dev))))
        ref, extra = peak_extra(lambda: torch_hist(*maps, grid_dev), B * (G + 1) * 8)
        got = interval_hist(*maps, grid)
        nbytes = 4 * 4 * npix * B
        bound = nbytes / HBM_BPS * 1e3
        h, t = med(ts["hip"]), med(ts["torch"])
        emit(dict(leg="fd_interval_hist_f32", data=data, repeat=rep, size=S, slices=B, G=G, air_share=round(air, 4) if data == "phantom" else 0.0,
                  bin0_share=round(float(got[:, 0].sum()) / (B * npix), 4), ms=round(h, 4), min_ms=round(min(ts["hip"]), 4),
                  ms_all=[round(v, 4) for v in ts["hip"]], MB=round(nbytes / 1e6, 2), GBps=round(nbytes / h / 1e6, 0),
                  bound_ms_at_6p3TBps=round(bound, 4), bound_over_ms=round(bound / h, 3), torch_ms=round(t, 4),
                  torch_over_hip=round(t / h, 3), torch_peak_extra_MB=round(extra / 1e6, 2), counts_equal_torch=bool(torch.equal(got, ref))))

    # leg 2: the scaled maps
    for data, maps in (("phantom", phantom), ("uniform", uniform)):
        ts = alternate((("hip", lambda: interval_scale(*maps[:3], 1.53125)), ("torch", lambda: torch_scale(*maps[:3], 1.53125))))
        ref, extra = peak_extra(lambda: torch_scale(*maps[:3], 1.53125), 2 * 4 * npix * B + 4 * B)
        got = interval_scale(*maps[:3], 1.53125)
        nbytes = 5 * 4 * npix * B
        bound = nbytes / HBM_BPS * 1e3
        h, t = med(ts["hip"]), med(ts["torch"])
        emit(dict(leg="fd_interval_scale_f32", data=data, size=S, slices=B, ms=round(h, 4), min_ms=round(min(ts["hip"]), 4),
                  MB=round(nbytes / 1e6, 2), GBps=round(nbytes / h / 1e6, 0), bound_ms_at_6p3TBps=round(bound, 4),
                  bound_over_ms=round(bound / h, 3), torch_ms=round(t, 4), torch_over_hip=round(t / h, 3),
                  torch_peak_extra_MB=round(extra / 1e6, 2), max_abs_diff_vs_torch=float(max((got[0] - ref[0]).abs().max(), (got[1] - ref[1]).abs().max())),
                  width_max_abs_diff_vs_torch=float((got[2] - ref[2]).abs().max())))
    del phantom, uniform
    torch.cuda.empty_cache()

    # leg 3: Trainer.calibrate_intervals against its own sampling
    if a.cal_slices > 0:
        from types import SimpleNamespace
        N, K = a.cal_slices, 8
        w = synth.synth_state_dict(arch.da_unet_spec(64, (1, 2, 4, 8), prefix=PREFIX), seed=0)
        net = UnetRes(dim=64, dim_mults=(1, 2, 4, 8), num_unet=1, condition=True, objective="pred_res", test_res_or_noise="res",
                      precision="bf16")
        dif = ResidualDiffusion(net, image_size=S, timesteps=1000, sampling_timesteps=2, objective="pred_res", loss_type="l2",
                                condition=True, sum_scale=0.01, test_res_or_noise="res")
        load_weights(dif, w, "synthetic weights")
        ds = SyntheticCTDataset(N, S)
        # synthetic weights predict nothing: a grid that reaches every finite score (|m - y| <= 1 over a half-width >= 1 / 3000)
        grid = np.concatenate([[0.0], np.geomspace(2.0 ** -4, 4096.0, 1024)]).astype(np.float32)
        with tempfile.TemporaryDirectory() as tmp:
            tr = Trainer(SimpleNamespace(is_train=False), dif, None, num_samples=1, condition=True, num_unet=1, checkpoint_folder=tmp,
                         is_train=False, dataset=ds, val_dataset=ds, device=dev)
            model = tr.ema.ema_model
            model.init()
            out = {}

            def plain():
                for i in range(N):
                    it = ds[i]
                    model.sample_ensemble([it[1][None].to(dev)], K, slice_seeds=[i], quantiles=LEVELS)

            legs = (("plain", plain),
                    ("calibrate", lambda: out.__setitem__("cal", tr.calibrate_intervals(n_samples=K, quantiles=LEVELS, alpha=0.1, grid=grid))))
            ms = {tag: [] for tag, _ in legs}
            for it in range(1 + a.reps):
                for tag, fn in legs:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    if it:
                        ms[tag].append((time.perf_counter() - t0) * 1e3)
            p, c = med(ms["plain"]), med(ms["calibrate"])
            cal = out["cal"]
            emit(dict(leg="calibrate_intervals", size=S, slices=N, K=K, ddim_steps=2, precision="bf16", levels=list(LEVELS), G=int(grid.size),
                      plain_ms=round(p, 2), calibrate_ms=round(c, 2), plain_ms_all=[round(v, 2) for v in ms["plain"]],
                      calibrate_ms_all=[round(v, 2) for v in ms["calibrate"]], calibrate_over_plain=round(c / p, 4), scale=cal.scale,
                      risk=cal.risk, raw_risk=cal.raw_risk))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(dict(tool="tools/interval_calibration_bench.py", size=S, slices=B, reps=a.reps, inner=a.inner, rows=rows)) + "\n")


if __name__ == "__main__":
    main()
