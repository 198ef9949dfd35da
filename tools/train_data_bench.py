"""The device-resident slice store (founddiff_amd.data.DeviceSliceStore, csrc/fd_train_data.hip): what feeding the training step from
HBM costs and saves.  Everything is reported, nothing is gated.  One JSON line per row:

  a  the fused entry alone at batch 2, 512 x 512: q_sample(StoreBatch) -- gather + flip / rot90 + normalize + x_res + q_sample + cat
     + times, keyed noise -- for code 0, a flip-only code (3: both flips, the register-reversed reads) and a transposing code
     (4: k = 1, the LDS tiles), against fd_res_qsample_f32 on an already assembled batch (q_sample on two tensors), and the gather
     alone.  ms, and GB/s over the bytes the launch must move: 2 images read, x_in (2), x_res and the noise written = 6 images
     (4 for the gather).
  b  wall milliseconds per step of Trainer.train over --steps steps (after --warm untimed ones) on the project's own model, dim 64,
     batch 2, 512 x 512, log_every off: from a SyntheticCTDataset (the host path: load, stack, three pageable uploads per
     micro-batch), and from a store built from it with augment off and on.  The three loops run in one process, one after the
     other, each from the same weights.

Milliseconds in a are medians of --reps timed calls after --warmup, the variants alternated call by call.

    python tools/train_data_bench.py [--batch 2] [--size 512] [--reps 20] [--warmup 3] [--steps 20] [--warm 3] [--legs a,b] [--out FILE]
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
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--items", type=int, default=16)
    ap.add_argument("--legs", default="a,b")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    from founddiff_amd import arch, diffusion_train as dt, synth
    from founddiff_amd.DADiff import ResidualDiffusion, Trainer, UnetRes, load_weights, residual_schedule
    from founddiff_amd.data import DeviceSliceStore, SyntheticCTDataset
    B, S = a.batch, a.size
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    ds = SyntheticCTDataset(a.items, S, seed=10)
    store = DeviceSliceStore.from_dataset(ds, dev)
    legs = a.legs.split(",")
    if "a" in legs:
        sch = residual_schedule(T)
        idx = list(range(B))
        t = np.arange(B, dtype=np.int64) * 37 % T
        seeds = np.arange(B, dtype=np.int64) + 7
        t_dev, seeds_dev = torch.from_numpy(t).to(dev), torch.from_numpy(seeds).to(dev)
        xs, xi = store.batch(idx)
        variants = [("assembled_fd_res_qsample_f32", 6, lambda: dt.q_sample(xs, xi, t_dev, sch, slice_seeds=seeds_dev, step=1))]
        for tag, code in (("store_code0", 0), ("store_flip_both", 3), ("store_transpose_k1", 4)):
            sb = dt.StoreBatch(store, idx, [code] * B)
            variants.append((tag, 6, lambda sb=sb: dt.q_sample(sb, None, t, sch, slice_seeds=seeds, step=1)))
            variants.append((tag + "_device_table", 6, lambda sb=sb: dt.q_sample(sb, None, t_dev, sch, slice_seeds=seeds_dev, step=1)))
            variants.append((tag + "_gather_only", 4, lambda code=code: store.batch(idx, [code] * B)))
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
        base = None
        for (tag, images, _), v in zip(variants, ts):
            ms = sorted(v)[len(v) // 2]
            base = ms if base is None else base
            nbytes = images * 4 * B * S * S
            emit(dict(leg="a_" + tag, batch=B, size=S, ms=round(ms, 4), min_ms=round(min(v), 4), MB=round(nbytes / 1e6, 2),
                      GBps=round(nbytes / ms / 1e6, 0), against_assembled=round(ms / base, 3)))
    if "b" in legs:
        w = synth.synth_state_dict(arch.da_unet_spec(64, (1, 2, 4, 8), prefix=PREFIX, clip=TINY_CLIP), seed=0)

        def loop(tag, train_dataset, augment):
            net = UnetRes(dim=64, dim_mults=(1, 2, 4, 8), num_unet=1, condition=True, objective="pred_res", test_res_or_noise="res",
                          precision="fp32", clip_cfg=TINY_CLIP)
            dif = ResidualDiffusion(net, image_size=S, timesteps=T, sampling_timesteps=2, objective="pred_res", loss_type="l1",
                                    condition=True, sum_scale=0.01, test_res_or_noise="res")
            load_weights(dif, w, "synthetic weights")
            with tempfile.TemporaryDirectory() as folder:
                tr = Trainer(None, dif.to(dev), checkpoint_folder=folder, dataset=ds, train_dataset=train_dataset, device=dev,
                             train_batch_size=B, gradient_accumulate_every=1, save_and_sample_every=10 ** 9, num_samples=1,
                             train_num_steps=a.warm, seed=5, log_every=0, augment=augment)
                tr.train()
                torch.cuda.synchronize()
                tr.train_num_steps = a.warm + a.steps
                t0 = time.perf_counter()
                tr.train()
                torch.cuda.synchronize()
                wall = (time.perf_counter() - t0) * 1e3 / a.steps
                loss = float(tr.losses[0])
            emit(dict(leg="b_" + tag, batch=B, size=S, steps=a.steps, ms_per_step=round(wall, 3), last_loss=round(loss, 6)))
            del tr, dif, net
            torch.cuda.empty_cache()
            return wall
        host = loop("trainer_host_dataset", ds, False)
        st0 = loop("trainer_store", store, False)
        st1 = loop("trainer_store_augment", store, True)
        host2 = loop("trainer_host_dataset_again", ds, False)
        emit(dict(leg="b_summary", host_ms=round(host, 3), host_again_ms=round(host2, 3), store_ms=round(st0, 3),
                  store_augment_ms=round(st1, 3), store_saves_ms=round(host - st0, 3), augment_costs_ms=round(st1 - st0, 3),
                  store_MB=round(store.nbytes / 1e6, 1)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(tool="tools/train_data_bench.py", batch=B, size=S, reps=a.reps, warmup=a.warmup, steps=a.steps, rows=rows), f,
                      indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
