"""Orientation ensembles (ResidualDiffusion.sample_ensemble(orientations=...), csrc/fd_ensemble_orient.hip): what the geometric
self-ensemble costs against the loop a caller had before and against the plain ensemble.  Everything is reported, nothing is gated.
The shipped architecture with synthetic weights, --size x --size slices, bf16, orientations "d4", one slice with K = 8 and eight
slices with K = 8, each at 2 and at 50 DDIM steps.  One row per (slices, K, steps): wall milliseconds per call to the closing
synchronisation, the legs alternated inside one loop, --reps timed rounds after one untimed round (which packs the engines and
captures the loop graphs), the median reported.  Inside a round every leg runs twice and its second call is timed: the first
sample_ensemble after a sample() of another batch size pays for the change (measured here: 22 ms at one slice, 130-160 ms at eight,
on whichever of ori and b follows a), which is a cost of alternating the legs and of neither leg:

  ori  sample_ensemble([x], K, slice_seeds, return_samples=True, orientations="d4")
  a    K calls of sample() on the torch-oriented slices (torch.flip / rot90 copies) under the replica seeds, the torch un-orient of
       every result and metrics.ensemble_stats: the tower K times per slice; its images and statistics are compared with ori's,
       bit for bit (`a_equals_ori`)
  b    plain sample_ensemble at the same K: the tower once per slice, so ori - b is the extra tower rows and the two transforms

with `peak_diff_ori` / `peak_diff_plain`, the largest difference between two replicas of a slice (un-oriented images, [0, 1] units)
in the orientation ensemble and in the plain one: the first holds the sampler's noise AND the model's non-equivariance, the
second the noise alone.

Then each new kernel alone, on random data of the same shapes, alternated in one loop with the composition it replaces, milliseconds
from device events around --inner back-to-back calls, the bytes the transform needs (not what either side moves) and those bytes
over 6.3 TB/s:

  fd_rows_orient_f32            against fd_rows_repeat_f32 and one torch.flip / rot90 copy per replica column
  fd_ensemble_orient_stats_f32  with and without the K un-oriented images, against one torch un-orient copy per replica column and
                                fd_ensemble_stats_f32
  fd_rows_take_f32              the conditioning rows of the replicas, against torch.index_select

    python tools/orientation_ensemble_bench.py [--size 512] [--reps 3] [--inner 20] [--steps 2,50] [--out FILE]
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
CASES = ((1, 8), (8, 8))               # (slices, K)


def turn(x, code):
    """the flip / rot90 code on the last two axes, with torch"""
    if code & 1:
        x = x.flip(-2)
    if code & 2:
        x = x.flip(-1)
    return torch.rot90(x, (code >> 2) & 3, (-2, -1)).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--steps", default="2,50")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "orientation_ensemble_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/orientation_ensemble_bench.py measures on the GPU: none is visible")
    dev = torch.device("cuda:0")
    from founddiff_amd import _lib as L
    from founddiff_amd import arch, synth
    from founddiff_amd.DADiff import ResidualDiffusion, UnetRes, load_weights
    from founddiff_amd.ensemble import ensemble_seeds, orientation_codes, orientation_inverse
    from founddiff_amd.metrics import ensemble_stats
    S = a.size
    npix = S * S
    rows = []
    med = lambda v: sorted(v)[len(v) // 2]
    stream = lambda: torch.cuda.current_stream().cuda_stream

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    def peak_diff(samples):            # (B, K, 1, H, W) -> the largest max_k - min_k over the pixels, per slice
        return [round(float(v), 6) for v in (samples.max(1).values - samples.min(1).values).flatten(1).max(1).values.cpu()]

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
            rs = torch.from_numpy(ensemble_seeds(seeds.numpy(), K))               # (B, K)
            codes = orientation_codes("d4", K, True).tolist()
            out = {}

            def ori():
                out["ori"] = dif.sample_ensemble([x], K, slice_seeds=seeds, return_samples=True, orientations="d4")

            def x_T(sd):               # the keyed x_T, given explicitly: sample() keys it on slice_seeds on some paths only
                return dif._keyed_noise(sd.contiguous().to(dev), dif.X_T_STEP, (sd.numel(), 1, S, S))

            def leg_a():
                imgs = [turn(dif.sample([turn(x, c)], batch_size=B, noise=x_T(rs[:, k]), slice_seeds=rs[:, k].contiguous())[-1],
                             orientation_inverse(c)) for k, c in enumerate(codes)]
                samples = torch.stack(imgs, 1)
                out["a"] = (samples,) + tuple(ensemble_stats(samples))

            def leg_b():
                out["b"] = dif.sample_ensemble([x], K, slice_seeds=seeds, return_samples=True)

            legs = (("ori", ori), ("a", leg_a), ("b", leg_b))
            ms = {tag: [] for tag, _ in legs}
            for it in range(1 + a.reps):
                for tag, fn in legs:
                    fn()                                                 # untimed: see the module's docstring
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    if it:
                        ms[tag].append((time.perf_counter() - t0) * 1e3)
            o, am, bm = med(ms["ori"]), med(ms["a"]), med(ms["b"])
            e = out["ori"]
            emit(dict(leg="sample_ensemble", orientations="d4", size=S, slices=B, K=K, ddim_steps=steps, precision="bf16",
                      ori_ms=round(o, 2), a_ms=round(am, 2), b_ms=round(bm, 2), ori_ms_all=[round(v, 2) for v in ms["ori"]],
                      a_ms_all=[round(v, 2) for v in ms["a"]], b_ms_all=[round(v, 2) for v in ms["b"]],
                      a_over_ori=round(am / o, 3), ori_over_b=round(o / bm, 3), ori_minus_b_ms=round(o - bm, 2),
                      a_equals_ori=bool(all(torch.equal(u, v) for u, v in zip(out["a"], (e.samples, e.mean, e.std, e.spread)))),
                      spread_ori=[round(float(v), 6) for v in e.spread.cpu()],
                      spread_plain=[round(float(v), 6) for v in out["b"].spread.cpu()],
                      peak_diff_ori=peak_diff(e.samples), peak_diff_plain=peak_diff(out["b"].samples)))
        del dif
        torch.cuda.empty_cache()

    # ---- the kernels alone, alternated with the compositions they replace
    def timed(fns):
        ts = {tag: [] for tag, _ in fns}
        for it in range(2 + a.reps):
            for tag, fn in fns:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.inner):
                    fn()
                e1.record()
                e1.synchronize()
                if it >= 2:
                    ts[tag].append(e0.elapsed_time(e1) / a.inner)
        return ts

    def report(leg, B, K, ts, nbytes, **extra):
        for tag, what, nb in nbytes:
            t = ts[tag]
            bound = nb / HBM_BPS * 1e3
            emit(dict(leg=leg, form=what, size=S, slices=B, K=K, ms=round(med(t), 4), min_ms=round(min(t), 4), MB=round(nb / 1e6, 2),
                      GBps=round(nb / med(t) / 1e6, 0), bound_ms_at_6p3TBps=round(bound, 4), bound_over_ms=round(bound / med(t), 3),
                      **extra))

    p = lambda t: t.data_ptr()
    for B, K in CASES:
        codes = orientation_codes("d4", K, True)
        inv = [orientation_inverse(c) for c in codes]
        c_dev = torch.from_numpy(codes).to(dev)
        i_dev = torch.tensor(inv, dtype=torch.int32, device=dev)
        g = torch.Generator().manual_seed(B * 10 + K)
        x = torch.rand(B, 1, S, S, generator=g).to(dev)
        dst, rep = torch.empty(B, K, 1, S, S, device=dev), torch.empty(B, K, 1, S, S, device=dev)

        def orient_hip():
            L.call("fd_rows_orient_f32", p(x), p(dst), p(c_dev), B, K, S, S, stream())

        def orient_torch():
            L.call("fd_rows_repeat_f32", p(x), p(rep), B, K, npix, stream())
            for k, c in enumerate(codes.tolist()):
                rep[:, k].copy_(turn(rep[:, k], c))
        ts = timed((("hip", orient_hip), ("torch", orient_torch)))
        nb = 4 * (B * npix + B * K * npix)
        report("fd_rows_orient_f32", B, K, ts, (("hip", "one launch (and the read-back of the K codes)", nb),
                                                ("torch", "fd_rows_repeat_f32 + a torch copy per replica column", nb)),
               equal=bool(torch.equal(dst, rep)))

        samples = torch.rand(B, K, npix, generator=g).to(dev)
        mean, std = torch.empty(B, npix, device=dev), torch.empty(B, npix, device=dev)
        ws, spread = torch.empty(B * L.lib().fd_ensemble_nblk(npix), device=dev), torch.empty(B, device=dev)
        un = torch.empty(B, K, npix, device=dev)
        ref = {}

        def stats_hip(with_samples):
            L.call("fd_ensemble_orient_stats_f32", p(samples), p(i_dev), p(mean), p(std), p(ws), p(spread),
                   p(un) if with_samples else None, B, K, S, S, stream())

        def stats_torch():
            t = torch.stack([turn(samples[:, k].view(B, S, S), c) for k, c in enumerate(inv)], 1).view(B, K, npix)
            ref["out"] = (t,) + tuple(ensemble_stats(t))
        ts = timed((("hip", lambda: stats_hip(False)), ("hip_samples", lambda: stats_hip(True)), ("torch", stats_torch)))
        stats_hip(True)
        equal = bool(all(torch.equal(u, v) for u, v in zip(ref["out"], (un, mean, std, spread))))
        sb, ob = 4 * B * K * npix, 4 * (2 * B * npix + B)
        report("fd_ensemble_orient_stats_f32", B, K, ts,
               (("hip", "mean, std, spread", sb + ob), ("hip_samples", "and the K un-oriented images", 2 * sb + ob),
                ("torch", "a torch un-orient copy per replica column + fd_ensemble_stats_f32", 2 * sb + ob)), equal=equal)

        D, n = 8, 1024                                                   # the rows of a time_dim-sized conditioning buffer
        tower = torch.rand(B * D, n, generator=g).to(dev)
        idx = torch.from_numpy((np.arange(B)[:, None] * D + np.arange(K)[None, :] % D).reshape(-1).astype(np.int32)).to(dev)
        idx64, rows_out = idx.long(), torch.empty(B * K, n, device=dev)
        ts = timed((("hip", lambda: L.call("fd_rows_take_f32", p(tower), p(rows_out), p(idx), B * K, n, stream())),
                    ("torch", lambda: torch.index_select(tower, 0, idx64, out=rows_out))))
        nb = 4 * 2 * B * K * n
        report("fd_rows_take_f32", B, K, ts, (("hip", "one launch", nb), ("torch", "torch.index_select", nb)), row_floats=n)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for row in rows:
                f.write(json.dumps(dict(tool="tools/orientation_ensemble_bench.py", reps=a.reps, inner=a.inner, **row)) + "\n")


if __name__ == "__main__":
    main()
