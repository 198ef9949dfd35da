"""Tiled sampling (ResidualDiffusion.sample_tiled, csrc/fd_tiles.hip): what a slice costs as overlapping tiles against sample() on
whole slices.  Everything is reported, nothing is gated.  The shipped architecture with synthetic weights, bf16, 2 and 50 DDIM
steps; wall milliseconds per call to the closing synchronisation, the legs alternated inside one loop, --reps timed rounds after one
untimed round (which packs the engines and captures the loop graphs), the median reported.  The whole-slice runs and the tiled runs
use two models with the same weights: an engine keeps one loop graph per kind, so one model alternating between two image sizes
would re-capture at every call.

  leg 1  512 x 512 slices at tile 256 / overlap 32 (3 x 3 tiles, 2.25 x the pixels), 1 and 8 slices: sample_tiled with
         condition="tile" and "slice" against sample() on the whole slices
  leg 2  one 1024 x 1024 slice at tile 512 / overlap 64 (3 x 3 tiles), condition="tile".  sample() on a whole slice of that size is
         not run here (no test of the library runs the engines there); the yardstick is sample() on four 512 x 512 slices, the same
         number of pixels
  leg 3  fd_tiles_gather_f32 and fd_tiles_blend_f32 alone at leg 1's plan with 8 slices: milliseconds from device events around
         --inner back-to-back calls, their bytes (gather: the tiles read and written; blend: the tiles read, the slices written) and
         those bytes over 6.3 TB/s

    python tools/tiled_bench.py [--reps 3] [--inner 20] [--steps 2,50] [--legs 1,2,3] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PREFIX = "model.unet0."
HBM_BPS = 6.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--steps", default="2,50")
    ap.add_argument("--legs", default="1,2,3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tiled_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/tiled_bench.py measures on the GPU: none is visible")
    dev = torch.device("cuda:0")
    from founddiff_amd import _lib as L
    from founddiff_amd import arch, synth
    from founddiff_amd.DADiff import ResidualDiffusion, UnetRes, load_weights
    rows = []
    legs_on = {int(v) for v in a.legs.split(",")}

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    w = synth.synth_state_dict(arch.da_unet_spec(64, (1, 2, 4, 8), prefix=PREFIX), seed=0)
    med = lambda v: sorted(v)[len(v) // 2]

    def model(steps, size):
        net = UnetRes(dim=64, dim_mults=(1, 2, 4, 8), num_unet=1, condition=True, objective="pred_res", test_res_or_noise="res",
                      precision="bf16")
        dif = ResidualDiffusion(net, image_size=size, timesteps=1000, sampling_timesteps=steps, objective="pred_res", loss_type="l2",
                                condition=True, sum_scale=0.01, test_res_or_noise="res")
        load_weights(dif, w, "synthetic weights")
        dif = dif.to(dev)
        dif.init()
        return dif

    def alternate(legs):
        ms = {tag: [] for tag, _ in legs}
        for it in range(1 + a.reps):
            for tag, fn in legs:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if it:
                    ms[tag].append((time.perf_counter() - t0) * 1e3)
        return ms

    for steps in [int(s) for s in a.steps.split(",")]:
        whole, tiled = model(steps, 512), model(steps, 512)
        if 1 in legs_on:
            for B in (1, 8):
                x = torch.from_numpy(synth.ct_phantom(B, 512, seed=10)[1]).to(dev)
                seeds = torch.arange(B, dtype=torch.int64) + 1000
                out = {}

                def leg_whole():
                    nz = whole._keyed_noise(seeds.to(dev), whole.X_T_STEP, tuple(x.shape))
                    out["whole"] = whole.sample([x], batch_size=B, noise=nz, slice_seeds=seeds)[-1]

                def leg_tile():
                    out["tile"] = tiled.sample_tiled([x], 256, 32, slice_seeds=seeds)[-1]

                def leg_slice():
                    out["slice"] = tiled.sample_tiled([x], 256, 32, slice_seeds=seeds, condition="slice")[-1]

                ms = alternate((("whole", leg_whole), ("tile", leg_tile), ("slice", leg_slice)))
                wm, tm, sm = med(ms["whole"]), med(ms["tile"]), med(ms["slice"])
                diff = lambda k: round(float((out[k] - out["whole"]).abs().mean()), 6)
                emit(dict(leg="sample_tiled_512", slices=B, tile=256, overlap=32, tiles_per_slice=9, pixel_ratio=2.25,
                          ddim_steps=steps, precision="bf16", whole_ms=round(wm, 2), tile_ms=round(tm, 2), slice_ms=round(sm, 2),
                          whole_ms_all=[round(v, 2) for v in ms["whole"]], tile_ms_all=[round(v, 2) for v in ms["tile"]],
                          slice_ms_all=[round(v, 2) for v in ms["slice"]], tile_over_whole=round(tm / wm, 3),
                          slice_over_whole=round(sm / wm, 3), mean_abs_diff_tile_vs_whole=diff("tile"),
                          mean_abs_diff_slice_vs_whole=diff("slice"),
                          workspace_MB_whole=round(sum(e.workspace_bytes() for e in whole.model.unet0._engine.values()) / 1e6, 0),
                          workspace_MB_tiled=round(sum(e.workspace_bytes() for e in tiled.model.unet0._engine.values()) / 1e6, 0)))
        if 2 in legs_on:
            big = model(steps, 1024)                               # tiles of 512 x 512: its own engines and graphs
            x1 = torch.from_numpy(synth.ct_phantom(1, 1024, seed=10)[1]).to(dev)
            x4 = torch.from_numpy(synth.ct_phantom(4, 512, seed=10)[1]).to(dev)
            s1, s4 = torch.tensor([1000], dtype=torch.int64), torch.arange(4, dtype=torch.int64) + 1000

            def leg_big():
                big.sample_tiled([x1], 512, 64, slice_seeds=s1)

            def leg_four():
                nz = whole._keyed_noise(s4.to(dev), whole.X_T_STEP, tuple(x4.shape))
                whole.sample([x4], batch_size=4, noise=nz, slice_seeds=s4)

            ms = alternate((("tiled", leg_big), ("four", leg_four)))
            tm, fm = med(ms["tiled"]), med(ms["four"])
            emit(dict(leg="sample_tiled_1024", slices=1, tile=512, overlap=64, tiles_per_slice=9, pixel_ratio=2.25, ddim_steps=steps,
                      precision="bf16", tiled_ms=round(tm, 2), four_512_slices_ms=round(fm, 2),
                      tiled_ms_all=[round(v, 2) for v in ms["tiled"]], four_ms_all=[round(v, 2) for v in ms["four"]],
                      tiled_over_four_512=round(tm / fm, 3), whole_1024_sample="not measured",
                      workspace_MB_tiled=round(sum(e.workspace_bytes() for e in big.model.unet0._engine.values()) / 1e6, 0)))
            del big
        del whole, tiled
        torch.cuda.empty_cache()
    if 3 in legs_on:
        from founddiff_amd.tiling import tile_plan, tile_weights
        import numpy as np
        B, H, W, th, tw, ov = 8, 512, 512, 256, 256, 32
        ys, xs = tile_plan(H, th, ov), tile_plan(W, tw, ov)
        my, mx = len(ys), len(xs)
        d = lambda v, dt: torch.from_numpy(np.ascontiguousarray(v.astype(dt))).to(dev)
        dys, dxs, dwy, dwx = d(ys, np.int32), d(xs, np.int32), d(tile_weights(ys, H, th), np.float32), d(tile_weights(xs, W, tw), np.float32)
        src = torch.rand(B, H * W, device=dev)
        tiles = torch.empty(B * my * mx, th * tw, device=dev)
        out = torch.empty(B, H * W, device=dev)
        st = torch.cuda.current_stream().cuda_stream
        x4f = int(bool((xs % 4 == 0).all()))
        calls = {
            "fd_tiles_gather_f32": (lambda: L.call("fd_tiles_gather_f32", src.data_ptr(), tiles.data_ptr(), dys.data_ptr(),
                                                   dxs.data_ptr(), B, H, W, th, tw, my, mx, x4f, st), 2 * tiles.numel() * 4),
            "fd_tiles_blend_f32": (lambda: L.call("fd_tiles_blend_f32", tiles.data_ptr(), dwy.data_ptr(), dwx.data_ptr(),
                                                  dys.data_ptr(), dxs.data_ptr(), out.data_ptr(), B, H, W, th, tw, my, mx, x4f, st),
                                   (tiles.numel() + out.numel()) * 4)}
        for name, (fn, nbytes) in calls.items():
            ts = []
            for it in range(2 + a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.inner):
                    fn()
                e1.record()
                e1.synchronize()
                if it >= 2:
                    ts.append(e0.elapsed_time(e1) / a.inner)
            bound = nbytes / HBM_BPS * 1e3
            emit(dict(leg=name, slices=B, size=512, tile=256, overlap=32, ms=round(med(ts), 4), min_ms=round(min(ts), 4),
                      MB=round(nbytes / 1e6, 2), GBps=round(nbytes / med(ts) / 1e6, 0), bound_ms_at_6p3TBps=round(bound, 4),
                      bound_over_ms=round(bound / med(ts), 3)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(dict(tool="tools/tiled_bench.py", reps=a.reps, inner=a.inner, rows=rows)) + "\n")


if __name__ == "__main__":
    main()
