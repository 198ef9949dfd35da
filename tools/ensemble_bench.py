"""Ensemble sampling (ResidualDiffusion.sample_ensemble, csrc/fd_ensemble.hip): what K keyed realisations per slice cost against
the two ways a caller had before.  Everything is reported, nothing is gated.  The shipped architecture with synthetic weights,
--size x --size slices, bf16, one slice with K = 8 and eight slices with K = 4, each at 2 and at 50 DDIM steps.  One row per
(slices, K, steps), wall milliseconds per call to the closing synchronisation, the legs alternated inside one loop, --reps timed
rounds after one untimed round (which packs the engines and captures the loop graphs), the median reported:

  ens  sample_ensemble([x], K, slice_seeds): the tower once per slice, the B K rows in passes of streams x max_sub_batch
  a    K calls of sample([x], slice_seeds=replica seeds k) on the B slices -- batch 1 for one slice --, the loop a caller writes
       without sample_ensemble: the tower K times per slice, and the one-slice shape when B = 1
  b    one sample() on the B K repeated rows under the replica seeds: the batched shape, the tower still K times per slice
       (a and b get the keyed x_T of the replica seeds as `noise=`: sample() keys x_T on slice_seeds on some of its paths only; their
       images are compared with the ensemble's, bit for bit: `a_equals_ens`, `b_equals_ens`)

and fd_ensemble_stats_f32 alone on the (B, K, size^2) stack: milliseconds from device events around --inner back-to-back calls,
its bytes -- K reads and two writes per pixel; the second pass over k re-reads from the L2 -- and those bytes over 6.3 TB/s.

    python tools/ensemble_bench.py [--size 512] [--reps 3] [--inner 20] [--steps 2,50] [--out FILE]
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
CASES = ((1, 8), (8, 4))               # (slices, K)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--steps", default="2,50")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/ensemble_bench.py measures on the GPU: none is visible")
    dev = torch.device("cuda:0")
    from founddiff_amd import arch, synth
    from founddiff_amd.DADiff import ResidualDiffusion, UnetRes, load_weights
    from founddiff_amd.ensemble import ensemble_seeds
    from founddiff_amd.metrics import ensemble_stats
    S = a.size
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    w = synth.synth_state_dict(arch.da_unet_spec(64, (1, 2, 4, 8), prefix=PREFIX), seed=0)
    net = UnetRes(dim=64, dim_mults=(1, 2, 4, 8), num_unet=1, condition=True, objective="pred_res", test_res_or_noise="res",
                  precision="bf16")
    med = lambda v: sorted(v)[len(v) // 2]
    step_list = [int(s) for s in a.steps.split(",")]
    for steps in step_list:
        dif = ResidualDiffusion(net, image_size=S, timesteps=1000, sampling_timesteps=steps, objective="pred_res", loss_type="l2",
                                condition=True, sum_scale=0.01, test_res_or_noise="res")
        load_weights(dif, w, "synthetic weights")
        dif = dif.to(dev)
        dif.init()
        for B, K in CASES:
            x = torch.from_numpy(synth.ct_phantom(B, S, seed=10)[1]).to(dev)
            seeds = torch.arange(B, dtype=torch.int64) + 1000
            rs = torch.from_numpy(ensemble_seeds(seeds.numpy(), K))               # (B, K)
            x_rep = x.repeat_interleave(K, 0)
            out = {}

            def ens():
                out["ens"] = dif.sample_ensemble([x], K, slice_seeds=seeds, return_samples=True)

            def x_T(sd):               # the keyed x_T, given explicitly: sample() keys it on slice_seeds on some paths only
                return dif._keyed_noise(sd.to(dev), dif.X_T_STEP, (sd.numel(), 1, S, S))

            def leg_a():
                out["a"] = [dif.sample([x], batch_size=B, noise=x_T(rs[:, k]), slice_seeds=rs[:, k].contiguous())[-1]
                            for k in range(K)]

            def leg_b():
                out["b"] = dif.sample([x_rep], batch_size=B * K, noise=x_T(rs.reshape(-1)), slice_seeds=rs.reshape(-1))[-1]

            legs = (("ens", ens), ("a", leg_a), ("b", leg_b))
            ms = {tag: [] for tag, _ in legs}
            for it in range(1 + a.reps):
                for tag, fn in legs:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    if it:
                        ms[tag].append((time.perf_counter() - t0) * 1e3)
            e, am, bm = med(ms["ens"]), med(ms["a"]), med(ms["b"])
            samples = out["ens"].samples
            emit(dict(leg="sample_ensemble", size=S, slices=B, K=K, ddim_steps=steps, precision="bf16",
                      ens_ms=round(e, 2), a_ms=round(am, 2), b_ms=round(bm, 2),
                      ens_ms_all=[round(v, 2) for v in ms["ens"]], a_ms_all=[round(v, 2) for v in ms["a"]],
                      b_ms_all=[round(v, 2) for v in ms["b"]], a_over_ens=round(am / e, 3), b_over_ens=round(bm / e, 3),
                      ens_ms_per_replica=round(e / (B * K), 2),
                      b_equals_ens=bool(torch.equal(out["b"], samples.reshape(out["b"].shape))),
                      a_equals_ens=bool(all(torch.equal(out["a"][k], samples[:, k]) for k in range(K))),
                      spread=[round(float(v), 6) for v in out["ens"].spread.cpu()]))
            if steps != step_list[0]:
                continue
            # the stats kernel alone, on this ensemble's images (once per case)
            ts = []
            for it in range(2 + a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.inner):
                    ensemble_stats(samples)
                e1.record()
                e1.synchronize()
                if it >= 2:
                    ts.append(e0.elapsed_time(e1) / a.inner)
            npix = S * S
            nbytes = 4 * (B * K * npix + 2 * B * npix + B)
            bound = nbytes / HBM_BPS * 1e3
            emit(dict(leg="fd_ensemble_stats_f32", size=S, slices=B, K=K, ms=round(med(ts), 4), min_ms=round(min(ts), 4),
                      MB=round(nbytes / 1e6, 2), GBps=round(nbytes / med(ts) / 1e6, 0), bound_ms_at_6p3TBps=round(bound, 4),
                      bound_over_ms=round(bound / med(ts), 3)))
        del dif
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(dict(tool="tools/ensemble_bench.py", size=S, reps=a.reps, inner=a.inner, rows=rows)) + "\n")


if __name__ == "__main__":
    main()
