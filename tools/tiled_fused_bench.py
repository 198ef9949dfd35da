"""Per-step fused tiled sampling (ResidualDiffusion.sample_tiled(fuse="step"), csrc/fd_tiles_step.hip) against the blend of final
images (fuse="final").  Everything is reported, nothing is gated.  The shipped architecture with synthetic weights, bf16, 512 x 512
slices at tile 256 / overlap 32 (3 x 3 tiles per slice), 1 and 8 slices, 2 and 50 DDIM steps.

  leg 1  wall milliseconds per call to the closing synchronisation of fuse="step" and fuse="final" on ONE model, alternated inside
         one loop, --reps timed rounds after one untimed round (which packs the engines and captures fuse="final"'s loop graphs),
         the median reported.  fuse="step" runs eagerly on one stream; fuse="final" replays captured loops on two.
         Two quality numbers on the synthetic model: the largest disagreement between overlapping tiles' final images in their
         common pixels under fuse="final" (under "step" the tiles hold the same bits there: tests/test_gpu_tiled_fused.py), and the
         relative L2 distance of each mode's image from sample() on the whole slices under the same x_T.
  leg 2  fd_tiles_step_ddim_f32 and fd_tiles_step_keyed_f32 alone at leg 1's plan with 8 slices, in place: milliseconds from device
         events around --inner back-to-back calls, their algorithmic bytes (every stream the mode touches once: the outputs read,
         x_t and x_in read, the rows written) and those bytes over 6.3 TB/s

    python tools/tiled_fused_bench.py [--reps 2] [--inner 20] [--steps 2,50] [--slices 1,8] [--legs 1,2] [--out FILE]
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
SIZE, TILE, OVERLAP = 512, 256, 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--steps", default="2,50")
    ap.add_argument("--slices", default="1,8")
    ap.add_argument("--legs", default="1,2")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tiled_fused_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/tiled_fused_bench.py measures on the GPU: none is visible")
    dev = torch.device("cuda:0")
    from founddiff_amd import _lib as L
    from founddiff_amd import arch, synth
    from founddiff_amd.DADiff import ResidualDiffusion, UnetRes, load_weights
    from founddiff_amd.tiling import tile_plan, tile_weights
    rows = []
    legs_on = {int(v) for v in a.legs.split(",")}
    ys, xs = tile_plan(SIZE, TILE, OVERLAP), tile_plan(SIZE, TILE, OVERLAP)
    my, mx = len(ys), len(xs)

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    w = synth.synth_state_dict(arch.da_unet_spec(64, (1, 2, 4, 8), prefix=PREFIX), seed=0)
    med = lambda v: sorted(v)[len(v) // 2]

    def model(steps):
        net = UnetRes(dim=64, dim_mults=(1, 2, 4, 8), num_unet=1, condition=True, objective="pred_res", test_res_or_noise="res",
                      precision="bf16")
        dif = ResidualDiffusion(net, image_size=SIZE, timesteps=1000, sampling_timesteps=steps, objective="pred_res", loss_type="l2",
                                condition=True, sum_scale=0.01, test_res_or_noise="res")
        load_weights(dif, w, "synthetic weights")
        dif = dif.to(dev)
        dif.init()
        return dif

    if 1 in legs_on:
        for steps in [int(s) for s in a.steps.split(",")]:
            whole, tiled = model(steps), model(steps)             # two models: an engine keeps one loop graph per kind and image size
            for B in [int(s) for s in a.slices.split(",")]:
                x = torch.from_numpy(synth.ct_phantom(B, SIZE, seed=10)[1]).to(dev)
                seeds = torch.arange(B, dtype=torch.int64) + 1000
                out, kept = {}, {}
                rows_of = tiled._tile_rows
                tiled._tile_rows = lambda *args: kept.__setitem__("tiles", rows_of(*args)) or kept["tiles"]
                ms = {"final": [], "step": []}
                for it in range(1 + a.reps):
                    for tag in ("final", "step"):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        out[tag] = tiled.sample_tiled([x], TILE, OVERLAP, slice_seeds=seeds, fuse=tag)[-1]
                        torch.cuda.synchronize()
                        if it:
                            ms[tag].append((time.perf_counter() - t0) * 1e3)
                del tiled._tile_rows
                nz = whole._keyed_noise(seeds.to(dev), whole.X_T_STEP, tuple(x.shape))
                ref = whole.sample([x], batch_size=B, noise=nz, slice_seeds=seeds)[-1]
                # the tiles' final images of fuse="final" in their common pixels: per pixel the largest minus the smallest cover
                t = kept["tiles"].view(B, my, mx, TILE, TILE)
                hi = torch.full((B, SIZE, SIZE), -float("inf"), device=dev)
                lo = torch.full((B, SIZE, SIZE), float("inf"), device=dev)
                for iy, ya in enumerate(ys):
                    for ix, xa in enumerate(xs):
                        win = (slice(None), slice(ya, ya + TILE), slice(xa, xa + TILE))
                        hi[win] = torch.maximum(hi[win], t[:, iy, ix])
                        lo[win] = torch.minimum(lo[win], t[:, iy, ix])
                l2 = lambda v: round(float((v - ref).double().norm() / ref.double().norm()), 6)
                fm, sm = med(ms["final"]), med(ms["step"])
                emit(dict(leg="sample_tiled_fused_512", slices=B, tile=TILE, overlap=OVERLAP, tiles_per_slice=my * mx, ddim_steps=steps,
                          precision="bf16", final_ms=round(fm, 2), step_ms=round(sm, 2), final_ms_all=[round(v, 2) for v in ms["final"]],
                          step_ms_all=[round(v, 2) for v in ms["step"]], step_over_final=round(sm / fm, 3),
                          max_tile_disagreement_final=round(float((hi - lo).max()), 6), max_tile_disagreement_step=0.0,
                          max_tile_disagreement_step_source="by construction: the tiles hold equal bits (tests/test_gpu_tiled_fused.py)",
                          l2_rel_final_vs_whole_sample=l2(out["final"]), l2_rel_step_vs_whole_sample=l2(out["step"]),
                          l2_rel_step_vs_final=round(float((out["step"] - out["final"]).double().norm() / out["final"].double().norm()), 6),
                          runs="one run on one MI355X"))
            del whole, tiled
            torch.cuda.empty_cache()
    if 2 in legs_on:
        B = 8
        R = B * my * mx
        d = lambda v, dt: torch.from_numpy(np.ascontiguousarray(v.astype(dt))).to(dev)
        dys, dxs = d(ys, np.int32), d(xs, np.int32)
        dwy, dwx = d(tile_weights(ys, SIZE, TILE), np.float32), d(tile_weights(xs, SIZE, TILE), np.float32)
        o0, o1 = torch.randn(R, TILE * TILE, device=dev), torch.randn(R, TILE * TILE, device=dev)
        img, x_in = torch.randn(R, TILE * TILE, device=dev) * 0.5, torch.rand(R, TILE * TILE, device=dev) * 2 - 1
        sl = torch.empty(B, SIZE * SIZE, device=dev)
        par = torch.tensor([0.5, 0.05, 0.5, 0.02, 0, 0, 0, 0], dtype=torch.float32, device=dev)
        tab = torch.tensor([[0.5, 0.05, 0.5, 0.9, 0.05, 0.05, -8.0, 0.0]] * 1000, dtype=torch.float32, device=dev)
        t_dev = torch.tensor([500], dtype=torch.int32, device=dev)
        seeds = (torch.arange(B, dtype=torch.int64) + 1000).to(dev)
        st = torch.cuda.current_stream().cuda_stream
        geom = (dwy.data_ptr(), dwx.data_ptr(), dys.data_ptr(), dxs.data_ptr(), B, SIZE, SIZE, TILE, TILE, my, mx,
                int(bool((xs % 4 == 0).all())))
        p = lambda v: None if v is None else v.data_ptr()

        def ddim(mode, a0, a1, xi, slc):
            return lambda: L.call("fd_tiles_step_ddim_f32", mode, p(a0), p(a1), img.data_ptr(), p(xi), par.data_ptr(), *geom,
                                  img.data_ptr(), p(slc), st)

        def keyed(mode, a0, a1, xi, slc):
            return lambda: L.call("fd_tiles_step_keyed_f32", mode, p(a0), p(a1), img.data_ptr(), p(xi), tab.data_ptr(), t_dev.data_ptr(),
                                  seeds.data_ptr(), *geom, img.data_ptr(), p(slc), 1000, st)
        row_bytes = img.numel() * 4
        calls = [("fd_tiles_step_ddim_f32", "mode 0 (o0, x_t, x_in -> rows)", ddim(0, o0, None, x_in, None), 4 * row_bytes),
                 ("fd_tiles_step_ddim_f32", "mode 0, last step (+ the slice image)", ddim(0, o0, None, x_in, sl), 4 * row_bytes + sl.numel() * 4),
                 ("fd_tiles_step_keyed_f32", "mode 0, t = 500 (o0, x_t, x_in -> rows, keyed noise)", keyed(0, o0, None, x_in, None), 4 * row_bytes),
                 ("fd_tiles_step_keyed_f32", "mode 2, t = 500 (o0, o1, x_t -> rows, keyed noise)", keyed(2, o0, o1, None, None), 4 * row_bytes)]
        for name, what, fn, nbytes in calls:
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
            emit(dict(leg=name, form=what, slices=B, size=SIZE, tile=TILE, overlap=OVERLAP, ms=round(med(ts), 4), min_ms=round(min(ts), 4),
                      MB=round(nbytes / 1e6, 2), GBps=round(nbytes / med(ts) / 1e6, 0), bound_ms_at_6p3TBps=round(bound, 4),
                      bound_over_ms=round(bound / med(ts), 3), runs="one run on one MI355X"))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(dict(tool="tools/tiled_fused_bench.py", reps=a.reps, inner=a.inner,
                                    note="every number is one run on one MI355X", rows=rows)) + "\n")


if __name__ == "__main__":
    main()
