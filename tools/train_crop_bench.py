"""Training on random crops (founddiff_amd.diffusion_train.StoreBatch(..., windows, crop), Trainer(crop_size=...),
csrc/fd_train_crop.hip): what a 256 x 256 patch out of a 512 x 512 store costs and saves.  Everything is reported, nothing is gated.
One JSON line per row:

  a  the fused crop launch alone at batch 2 and 8: q_sample(StoreBatch(..., windows, crop)) -- crop + flip / rot90 + normalize +
     x_res + q_sample + cat + times, keyed noise -- for code 0, code 2 (a W flip: the register-reversed reads) and code 4 (k = 1,
     the LDS tiles), each with every window at x0 % 4 == 0 (the source reads happen to be 16-byte aligned) and at x0 % 4 == 1
     (they never are), against fd_store_crop_f32 followed by fd_res_qsample_f32 (store.batch(...) then q_sample on two tensors:
     two launches and an assembled batch) and against the uncropped fd_res_qsample_store_f32 on the same items.  ms, and GB/s over
     the bytes the launch must move: 2 images read, x_in (2), x_res and the noise written = 6 images of the OUTPUT size.
  b  wall milliseconds per step of Trainer.train over --steps steps (after --warm untimed ones) on the project's own model, dim 64,
     from one store, augment on, log_every off: whole 512 x 512 slices at batch 2, 256 x 256 crops at batch 2 and at batch 8.  The
     loops run in one process, one after the other, each from the same weights; the first is repeated at the end.

Milliseconds in a are medians of --reps timed calls after --warmup, the variants alternated call by call.

    python tools/train_crop_bench.py [--size 512] [--crop 256] [--reps 20] [--warmup 3] [--steps 20] [--warm 3] [--legs a,b] [--out FILE]
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

T = 1000
TINY_CLIP = dict(layers=(2, 1, 1, 1), width=16, embed_dim=1024)
PREFIX = "model.unet0."


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--crop", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--items", type=int, default=16)
    ap.add_argument("--legs", default="a,b")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_crop_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    from founddiff_amd import arch, diffusion_train as dt, synth
    from founddiff_amd.DADiff import ResidualDiffusion, Trainer, UnetRes, load_weights, residual_schedule
    from founddiff_amd.data import DeviceSliceStore, SyntheticCTDataset
    S, C = a.size, a.crop
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    ds = SyntheticCTDataset(a.items, S, seed=10)
    store = DeviceSliceStore.from_dataset(ds, dev)
    legs = a.legs.split(",")
    if "a" in legs:
        sch = residual_schedule(T)
        for B in (2, 8):
            idx = [k % a.items for k in range(B)]
            t = np.arange(B, dtype=np.int64) * 37 % T
            seeds = np.arange(B, dtype=np.int64) + 7
            t_dev, seeds_dev = torch.from_numpy(t).to(dev), torch.from_numpy(seeds).to(dev)
            whole = dt.StoreBatch(store, idx, [0] * B)
            variants = [("uncropped_fd_res_qsample_store_f32", S, lambda: dt.q_sample(whole, None, t, sch, slice_seeds=seeds, step=1))]
            for code in (0, 2, 4):
                for xm in (0, 1):
                    win = [[4 * (5 * k % 16) + 8, 4 * (7 * k % 16) + xm] for k in range(B)]
                    codes = [code] * B
                    sb = dt.StoreBatch(store, idx, codes, win, C)
                    variants.append((f"crop_code{code}_x0mod4_{xm}", C, lambda sb=sb: dt.q_sample(sb, None, t, sch, slice_seeds=seeds, step=1)))

                    def composed(codes=codes, win=win):
                        xs, xi = store.batch(idx, codes, win, C)
                        return dt.q_sample(xs, xi, t_dev, sch, slice_seeds=seeds_dev, step=1)
                    variants.append((f"crop_code{code}_x0mod4_{xm}_composed", C, composed))
            ts = [[] for _ in variants]
            for it in range(a.warmup + a.reps):
                for i, (_, _, fn) in enumerate(variants):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    e1.synchronize()
                    if it >= a.warmup:
                        ts[i].append(e0.elapsed_time(e1))
            med = {tag: sorted(v)[len(v) // 2] for (tag, _, _), v in zip(variants, ts)}
            for (tag, side, _), v in zip(variants, ts):
                ms = med[tag]
                nbytes = 6 * 4 * B * side * side
                row = dict(leg="a_" + tag, batch=B, size=S, out=side, ms=round(ms, 4), min_ms=round(min(v), 4), MB=round(nbytes / 1e6, 2),
                           GBps=round(nbytes / ms / 1e6, 0), against_uncropped=round(ms / med["uncropped_fd_res_qsample_store_f32"], 3))
                if tag.startswith("crop") and not tag.endswith("_composed"):
                    row["against_composed"] = round(ms / med[tag + "_composed"], 3)
                emit(row)
    if "b" in legs:
        w = synth.synth_state_dict(arch.da_unet_spec(64, (1, 2, 4, 8), prefix=PREFIX, clip=TINY_CLIP), seed=0)

        def loop(tag, B, crop):
            net = UnetRes(dim=64, dim_mults=(1, 2, 4, 8), num_unet=1, condition=True, objective="pred_res", test_res_or_noise="res",
                          precision="fp32", clip_cfg=TINY_CLIP)
            dif = ResidualDiffusion(net, image_size=S, timesteps=T, sampling_timesteps=2, objective="pred_res", loss_type="l1",
                                    condition=True, sum_scale=0.01, test_res_or_noise="res")
            load_weights(dif, w, "synthetic weights")
            with tempfile.TemporaryDirectory() as folder:
                tr = Trainer(None, dif.to(dev), checkpoint_folder=folder, dataset=ds, train_dataset=store, device=dev,
                             train_batch_size=B, gradient_accumulate_every=1, save_and_sample_every=10 ** 9, num_samples=1,
                             train_num_steps=a.warm, seed=5, log_every=0, augment=True, crop_size=crop)
                tr.train()
                torch.cuda.synchronize()
                tr.train_num_steps = a.warm + a.steps
                t0 = time.perf_counter()
                tr.train()
                torch.cuda.synchronize()
                wall = (time.perf_counter() - t0) * 1e3 / a.steps
                loss = float(tr.losses[0])
            emit(dict(leg="b_" + tag, batch=B, size=S, crop=crop, steps=a.steps, ms_per_step=round(wall, 3),
                      ms_per_item=round(wall / B, 3), last_loss=round(loss, 6)))
            del tr, dif, net
            torch.cuda.empty_cache()
            return wall
        full = loop("trainer_whole_b2", 2, None)
        c2 = loop(f"trainer_crop{C}_b2", 2, C)
        c8 = loop(f"trainer_crop{C}_b8", 8, C)
        full2 = loop("trainer_whole_b2_again", 2, None)
        emit(dict(leg="b_summary", whole_b2_ms=round(full, 3), whole_b2_again_ms=round(full2, 3), crop_b2_ms=round(c2, 3),
                  crop_b8_ms=round(c8, 3), crop_b2_over_whole_b2=round(c2 / full, 3), crop_b8_over_whole_b2=round(c8 / full, 3)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(dict(tool="tools/train_crop_bench.py", size=S, crop=C, reps=a.reps, warmup=a.warmup, steps=a.steps,
                                    warm=a.warm, rows=rows)) + "\n")


if __name__ == "__main__":
    main()
