"""Ensemble quantiles (ResidualDiffusion.sample_ensemble(quantiles=...), csrc/fd_ensemble_order.hip): what the per-pixel order
statistics of K realisations cost.  Everything is reported, nothing is gated.  --size x --size slices, bf16 model, one JSON line per
case:

  leg 1  fd_ensemble_order_f32 alone on random (B, K, size^2) images, Q = 3 levels (0.05, 0.5, 0.95): 1 slice x K = 8 and 8 slices x
         K = 4 (the sorting networks), 1 slice x K = 32 (the largest network) and 1 slice x K = 33 (the counting path), alternated
         with torch.quantile on the same device tensor.  Milliseconds from device events around --inner back-to-back calls, the
         median of --reps rounds after two untimed ones; the kernel's bytes (K + Q) 4 n per slice, those bytes per second and over 6.3 TB/s; torch's time over the kernel's;
         torch.quantile's peak extra device memory (it sorts a copy); the largest difference between the two, and of each from
         numpy's float64 quantile of the same values.
  leg 2  sample_ensemble with and without quantiles=(0.05, 0.5, 0.95) on the shipped architecture with synthetic weights, 1 slice x
         K = 8 and 8 slices x K = 4 at 2 and at 50 DDIM steps: wall milliseconds per call to the closing synchronisation, alternated,
         the median of --reps rounds after one untimed round.

    python tools/ensemble_quantiles_bench.py [--size 512] [--reps 3] [--inner 20] [--steps 2,50] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PREFIX = "model.unet0."
HBM_BPS = 6.3e12
LEVELS = (0.05, 0.5, 0.95)
KERNEL_CASES = ((1, 8), (8, 4), (1, 32), (1, 33))        # (slices, K); K = 32: the largest network, K = 33: the counting path
CASES = ((1, 8), (8, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--steps", default="2,50")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble_quantiles_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/ensemble_quantiles_bench.py measures on the GPU: none is visible")
    dev = torch.device("cuda:0")
    from founddiff_amd import arch, synth
    from founddiff_amd.DADiff import ResidualDiffusion, UnetRes, load_weights
    from founddiff_amd.metrics import ensemble_quantiles
    S = a.size
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

    # leg 1: the order kernel alone against torch.quantile
    q_t = torch.tensor(LEVELS, device=dev)
    for B, K in KERNEL_CASES:
        x = torch.rand(B, K, npix, generator=torch.Generator().manual_seed(K)).to(dev)
        legs = (("hip", lambda: ensemble_quantiles(x, LEVELS)), ("torch", lambda: torch.quantile(x, q_t, dim=1)))
        ts = {tag: [] for tag, _ in legs}
        for it in range(2 + a.reps):
            for tag, fn in legs:
                t = timed(fn)
                if it >= 2:
                    ts[tag].append(t)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        ref = torch.quantile(x, q_t, dim=1)                                  # (Q, B, n)
        torch.cuda.synchronize()
        extra = torch.cuda.max_memory_allocated() - base - ref.numel() * 4
        got = ensemble_quantiles(x, LEVELS)
        err = float((got - ref.permute(1, 0, 2)).abs().max())
        # both against numpy's float64 quantile of the same values (torch places the level, q (K - 1), in float32)
        ref64 = np.quantile(x.cpu().numpy().astype(np.float64), LEVELS, axis=1)        # (Q, B, n)
        hip64 = float(np.abs(got.permute(1, 0, 2).cpu().numpy() - ref64).max())
        torch64 = float(np.abs(ref.cpu().numpy() - ref64).max())
        nbytes = 4 * (K + len(LEVELS)) * npix * B
        bound = nbytes / HBM_BPS * 1e3
        h, t = med(ts["hip"]), med(ts["torch"])
        emit(dict(leg="fd_ensemble_order_f32", path="networks" if K <= 32 else "counting", size=S, slices=B, K=K, Q=len(LEVELS),
                  ms=round(h, 4), min_ms=round(min(ts["hip"]), 4), MB=round(nbytes / 1e6, 2), GBps=round(nbytes / h / 1e6, 0),
                  bound_ms_at_6p3TBps=round(bound, 4), bound_over_ms=round(bound / h, 3), torch_quantile_ms=round(t, 4),
                  torch_over_hip=round(t / h, 3), torch_peak_extra_MB=round(extra / 1e6, 2), max_abs_diff_vs_torch=err,
                  max_abs_err_vs_float64=hip64, torch_max_abs_err_vs_float64=torch64))
        del x, ref, got

    # leg 2: sample_ensemble with and without the levels
    w = synth.synth_state_dict(arch.da_unet_spec(64, (1, 2, 4, 8), prefix=PREFIX), seed=0)
    net = UnetRes(dim=64, dim_mults=(1, 2, 4, 8), num_unet=1, condition=True, objective="pred_res", test_res_or_noise="res",
                  precision="bf16")
    for steps in [int(s) for s in a.steps.split(",")]:
        dif = ResidualDiffusion(net, image_size=S, timesteps=1000, sampling_timesteps=steps, objective="pred_res", loss_type="l2",
                                condition=True, sum_scale=0.01, test_res_or_noise="res")
        load_weights(dif, w, "synthetic weights")
        dif = dif.to(dev)
        dif.init()
        for B, K in CASES:
            x = torch.from_numpy(synth.ct_phantom(B, S, seed=10)[1]).to(dev)
            seeds = torch.arange(B, dtype=torch.int64) + 1000
            out = {}
            legs = (("plain", lambda: out.__setitem__("plain", dif.sample_ensemble([x], K, slice_seeds=seeds))),
                    ("quant", lambda: out.__setitem__("quant", dif.sample_ensemble([x], K, slice_seeds=seeds, quantiles=LEVELS))))
            ms = {tag: [] for tag, _ in legs}
            for it in range(1 + a.reps):
                for tag, fn in legs:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    if it:
                        ms[tag].append((time.perf_counter() - t0) * 1e3)
            p, q = med(ms["plain"]), med(ms["quant"])
            emit(dict(leg="sample_ensemble_quantiles", size=S, slices=B, K=K, ddim_steps=steps, precision="bf16", levels=list(LEVELS),
                      plain_ms=round(p, 2), quantiles_ms=round(q, 2), plain_ms_all=[round(v, 2) for v in ms["plain"]],
                      quantiles_ms_all=[round(v, 2) for v in ms["quant"]], quantiles_over_plain=round(q / p, 4),
                      mean_equal=bool(torch.equal(out["plain"].mean, out["quant"].mean)),
                      std_equal=bool(torch.equal(out["plain"].std, out["quant"].std))))
        del dif
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(dict(tool="tools/ensemble_quantiles_bench.py", size=S, reps=a.reps, inner=a.inner, rows=rows)) + "\n")


if __name__ == "__main__":
    main()
