"""Tiled ensembles (ResidualDiffusion.sample_ensemble(tile=...), csrc/fd_tiles_ensemble.hip): what K keyed realisations of a slice
sampled as tiles cost against the two ways a caller had before.  Everything is reported, nothing is gated.  The shipped architecture
with synthetic weights, bf16, 512 x 512 slices at tile 256 / overlap 32 (3 x 3 tiles per slice), one slice with K = 8 and eight slices
with K = 4, each at 2 and at 50 DDIM steps, for tile_fuse "final" and "step".

  leg 1  one row per (fuse, slices, K, steps): wall milliseconds per call to the closing synchronisation, the legs alternated inside
         one loop, --reps timed rounds after one untimed round (which packs the engines, captures the loop graphs, counts the rows
         the DA-CLIP tower saw and keeps the images that are compared), the median reported:
           ens  sample_ensemble([x], K, slice_seeds, tile=..., tile_fuse=fuse): the tower once per slice and tile
           a    K calls of sample_tiled([x], slice_seeds=replica seeds k, fuse=fuse): the tower K times per tile
           b    sample_tiled on the B K repeated slices under the replica seeds, then ensemble_stats on its images: the batched
                shape, the tower still K times per tile, K whole-slice images written and read again
         `a_equals_ens`, `b_equals_ens`: the replicas' images bit for bit; `b_stats_equal_ens`: mean, std and spread bit for bit.
  leg 2  fd_tiles_ensemble_f32 alone (with and without the K blended images) against fd_tiles_blend_f32 + fd_ensemble_stats_f32 on
         the same tiles: milliseconds from device events around --inner back-to-back calls, the algorithmic bytes (the tiles read
         once, mean and std written, the images written -- and for blend + stats read again -- where they exist) and those bytes
         over 6.3 TB/s.  The second pass over k re-reads the tiles from the caches in one form and the images in the other.

    python tools/tiled_ensemble_bench.py [--reps 2] [--inner 20] [--steps 2,50] [--fuse final,step] [--legs 1,2] [--out FILE]
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
CASES = ((1, 8), (8, 4))               # (slices, K)
RUNS = "one run on one MI355X"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--steps", default="2,50")
    ap.add_argument("--fuse", default="final,step")
    ap.add_argument("--legs", default="1,2")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tiled_ensemble_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/tiled_ensemble_bench.py measures on the GPU: none is visible")
    dev = torch.device("cuda:0")
    from founddiff_amd import _lib as L
    from founddiff_amd import arch, synth
    from founddiff_amd.DADiff import ResidualDiffusion, UnetRes, load_weights
    from founddiff_amd.engine import DAEngine
    from founddiff_amd.ensemble import ensemble_seeds
    from founddiff_amd.metrics import ensemble_stats
    from founddiff_amd.tiling import tile_plan, tile_weights
    rows = []
    legs_on = {int(v) for v in a.legs.split(",")}
    ys, xs = tile_plan(SIZE, TILE, OVERLAP), tile_plan(SIZE, TILE, OVERLAP)
    my, mx = len(ys), len(xs)
    T = my * mx

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    med = lambda v: sorted(v)[len(v) // 2]
    tower = {"rows": 0}
    real = DAEngine.encode_dose

    def counting(self, x_cond):
        tower["rows"] += x_cond.shape[0]
        return real(self, x_cond)
    DAEngine.encode_dose = counting

    if 1 in legs_on:
        w = synth.synth_state_dict(arch.da_unet_spec(64, (1, 2, 4, 8), prefix=PREFIX), seed=0)
        net = UnetRes(dim=64, dim_mults=(1, 2, 4, 8), num_unet=1, condition=True, objective="pred_res", test_res_or_noise="res",
                      precision="bf16")
        for steps in [int(s) for s in a.steps.split(",")]:
            dif = ResidualDiffusion(net, image_size=SIZE, timesteps=1000, sampling_timesteps=steps, objective="pred_res",
                                    loss_type="l2", condition=True, sum_scale=0.01, test_res_or_noise="res")
            load_weights(dif, w, "synthetic weights")
            dif = dif.to(dev)
            dif.init()
            for fuse in a.fuse.split(","):
                for B, K in CASES:
                    x = torch.from_numpy(synth.ct_phantom(B, SIZE, seed=10)[1]).to(dev)
                    seeds = torch.arange(B, dtype=torch.int64) + 1000
                    rs = torch.from_numpy(ensemble_seeds(seeds.numpy(), K))           # (B, K)
                    x_rep = x.repeat_interleave(K, 0)
                    out = {}

                    def ens(keep):
                        out["ens"] = dif.sample_ensemble([x], K, slice_seeds=seeds, return_samples=keep, tile=TILE, overlap=OVERLAP,
                                                         tile_fuse=fuse)

                    def leg_a(keep):
                        out["a"] = [dif.sample_tiled([x], TILE, OVERLAP, slice_seeds=rs[:, k].contiguous(), fuse=fuse)[-1]
                                    for k in range(K)]

                    def leg_b(keep):
                        img = dif.sample_tiled([x_rep], TILE, OVERLAP, slice_seeds=rs.reshape(-1), fuse=fuse)[-1]
                        out["b"] = (img, ensemble_stats(img.view(B, K, 1, SIZE, SIZE)))

                    legs = (("ens", ens), ("a", leg_a), ("b", leg_b))
                    ms = {tag: [] for tag, _ in legs}
                    seen, eq = {}, {}
                    for it in range(1 + a.reps):
                        for tag, fn in legs:
                            tower["rows"] = 0
                            torch.cuda.synchronize()
                            t0 = time.perf_counter()
                            fn(it == 0)                        # the untimed round keeps the ensemble's images for the comparison
                            torch.cuda.synchronize()
                            if it:
                                ms[tag].append((time.perf_counter() - t0) * 1e3)
                            else:
                                seen[tag] = tower["rows"]
                        if it == 0:
                            e, (img, (mean, std, spread)) = out["ens"], out["b"]
                            eq = dict(a_equals_ens=bool(all(torch.equal(out["a"][k], e.samples[:, k]) for k in range(K))),
                                      b_equals_ens=bool(torch.equal(img, e.samples.reshape(img.shape))),
                                      b_stats_equal_ens=bool(torch.equal(mean, e.mean) and torch.equal(std, e.std) and
                                                             torch.equal(spread, e.spread)),
                                      spread=[round(float(v), 6) for v in e.spread.cpu()])
                    em, am, bm = med(ms["ens"]), med(ms["a"]), med(ms["b"])
                    emit(dict(leg="sample_ensemble_tiled_512", fuse=fuse, slices=B, K=K, tile=TILE, overlap=OVERLAP, tiles_per_slice=T,
                              ddim_steps=steps, precision="bf16", ens_ms=round(em, 2), a_ms=round(am, 2), b_ms=round(bm, 2),
                              ens_ms_all=[round(v, 2) for v in ms["ens"]], a_ms_all=[round(v, 2) for v in ms["a"]],
                              b_ms_all=[round(v, 2) for v in ms["b"]], a_over_ens=round(am / em, 3), b_over_ens=round(bm / em, 3),
                              tower_rows_ens=seen["ens"], tower_rows_a=seen["a"], tower_rows_b=seen["b"], **eq, runs=RUNS))
            del dif
            torch.cuda.empty_cache()
    if 2 in legs_on:
        d = lambda v, dt: torch.from_numpy(np.ascontiguousarray(v.astype(dt))).to(dev)
        dys, dxs = d(ys, np.int32), d(xs, np.int32)
        dwy, dwx = d(tile_weights(ys, SIZE, TILE), np.float32), d(tile_weights(xs, SIZE, TILE), np.float32)
        x4 = int(bool((xs % 4 == 0).all()))
        st = torch.cuda.current_stream().cuda_stream
        npix = SIZE * SIZE
        for B, K in CASES:
            tiles = torch.rand(B * K * T, TILE * TILE, device=dev)
            samples = torch.empty(B, K, npix, device=dev)
            mean, std = torch.empty(B, npix, device=dev), torch.empty(B, npix, device=dev)
            ws, spread = torch.empty(B * L.lib().fd_ensemble_nblk(npix), device=dev), torch.empty(B, device=dev)
            plan = (dwy.data_ptr(), dwx.data_ptr(), dys.data_ptr(), dxs.data_ptr())

            def fused(sp):
                return lambda: L.call("fd_tiles_ensemble_f32", tiles.data_ptr(), *plan, sp, mean.data_ptr(), std.data_ptr(),
                                      ws.data_ptr(), spread.data_ptr(), B, K, SIZE, SIZE, TILE, TILE, my, mx, x4, st)

            def two():
                L.call("fd_tiles_blend_f32", tiles.data_ptr(), *plan, samples.data_ptr(), B * K, SIZE, SIZE, TILE, TILE, my, mx, x4, st)
                L.call("fd_ensemble_stats_f32", samples.data_ptr(), mean.data_ptr(), std.data_ptr(), ws.data_ptr(), spread.data_ptr(),
                       B, K, npix, st)
            tb, sb, ob = tiles.numel() * 4, samples.numel() * 4, 2 * B * npix * 4 + B * 4
            calls = [("fd_tiles_ensemble_f32", "samples = NULL (tiles -> mean, std, spread)", fused(None), tb + ob),
                     ("fd_tiles_ensemble_f32", "with the K blended images written", fused(samples.data_ptr()), tb + sb + ob),
                     ("fd_tiles_blend_f32 + fd_ensemble_stats_f32", "the images written, then read", two, tb + 2 * sb + ob)]
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
                emit(dict(leg=name, form=what, slices=B, K=K, size=SIZE, tile=TILE, overlap=OVERLAP, ms=round(med(ts), 4),
                          min_ms=round(min(ts), 4), MB=round(nbytes / 1e6, 2), GBps=round(nbytes / med(ts) / 1e6, 0),
                          bound_ms_at_6p3TBps=round(bound, 4), bound_over_ms=round(bound / med(ts), 3), runs=RUNS))
    DAEngine.encode_dose = real
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(dict(tool="tools/tiled_ensemble_bench.py", reps=a.reps, inner=a.inner,
                                    note="every number is one run on one MI355X", rows=rows)) + "\n")


if __name__ == "__main__":
    main()
