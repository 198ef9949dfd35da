"""Validation during training (Trainer.validate, ResidualDiffusion.eval_items, csrc/fd_validate.hip): what one held-out evaluation
costs.  Everything is reported, nothing is gated.  One JSON line per row:

  a  wall milliseconds per Trainer.validate() on the project's own model, dim 64, --size x --size slices, --items items x 4 noise
     bands in batches of --batch (item, band) pairs, from a device store: on the fp32 engine (the default) and on the bf16
     engine, alternated, --reps timed calls each after one untimed call (which packs the engine), every call ending in the
     synchronisation validate() ends in anyway.  The weights do not change between calls, so this is the evaluation alone,
     without the repacking of the engine that follows an optimiser step.
  b  fd_val_items_f32 alone (diffusion_train.val_items: its three launches and the workspace) at the validation's batch and at 64
     slices: milliseconds per call from device events around --inner back-to-back calls, median of --reps; its bytes -- 4 streams
     read, 2 B floats written -- and those bytes over 6.3 TB/s, the bound the other training tools use.  At the validation's batch
     the four inputs fit the Infinity Cache, so a rate above HBM's is no contradiction.

    python tools/validate_bench.py [--size 512] [--items 64] [--batch 8] [--reps 3] [--inner 20] [--legs a,b] [--out FILE]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T = 1000
TINY_CLIP = dict(layers=(2, 1, 1, 1), width=16, embed_dim=1024)
PREFIX = "model.unet0."
BANDS = (0, 250, 500, 750, 1000)
HBM_BPS = 6.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--items", type=int, default=64)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--legs", default="a,b")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "validate_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/validate_bench.py measures on the GPU: none is visible")
    dev = torch.device("cuda:0")
    from founddiff_amd import arch, diffusion_train as dt, synth
    from founddiff_amd.DADiff import ResidualDiffusion, Trainer, UnetRes, load_weights
    from founddiff_amd.data import DeviceSliceStore, SyntheticCTDataset
    S = a.size
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    legs = a.legs.split(",")
    if "a" in legs:
        ds = SyntheticCTDataset(a.items, S, seed=11)
        store = DeviceSliceStore.from_dataset(ds, dev)
        w = synth.synth_state_dict(arch.da_unet_spec(64, (1, 2, 4, 8), prefix=PREFIX, clip=TINY_CLIP), seed=0)
        net = UnetRes(dim=64, dim_mults=(1, 2, 4, 8), num_unet=1, condition=True, objective="pred_res", test_res_or_noise="res",
                      precision="bf16", clip_cfg=TINY_CLIP)
        dif = ResidualDiffusion(net, image_size=S, timesteps=T, sampling_timesteps=2, objective="pred_res", loss_type="l1",
                                condition=True, sum_scale=0.01, test_res_or_noise="res")
        load_weights(dif, w, "synthetic weights")
        with tempfile.TemporaryDirectory() as folder:
            tr = Trainer(None, dif.to(dev), checkpoint_folder=folder, dataset=store, device=dev, num_samples=1, val_dataset=store,
                         val_bands=BANDS, val_batch_size=a.batch, val_seed=0)
            modes = (("fp32", "fp32"), ("bf16", None))                   # None: the model's sampling precision
            ms = {tag: [] for tag, _ in modes}
            last = {}
            for it in range(1 + a.reps):
                for tag, prec in modes:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    last[tag] = tr.validate(precision=prec)
                    torch.cuda.synchronize()
                    if it:
                        ms[tag].append((time.perf_counter() - t0) * 1e3)
            pairs = a.items * (len(BANDS) - 1)
            for tag, _ in modes:
                v = sorted(ms[tag])
                emit(dict(leg="a_validate_" + tag, size=S, items=a.items, bands=len(BANDS) - 1, batch=a.batch, forwards=pairs,
                          ms=round(v[len(v) // 2], 2), min_ms=round(v[0], 2), max_ms=round(v[-1], 2),
                          ms_per_forward=round(v[len(v) // 2] / pairs, 3), loss=[round(x, 6) for x in last[tag]["loss"][0]],
                          psnr=[round(x, 4) for x in last[tag]["psnr"][0]]))
            del tr
        del dif, net, store
        torch.cuda.empty_cache()
    if "b" in legs:
        npix = S * S
        for B in sorted({a.batch, 64}):
            g = torch.Generator().manual_seed(B)
            pred, target = 1.5 * torch.randn(B, 1, S, S, generator=g).to(dev), torch.randn(B, 1, S, S, generator=g).to(dev)
            x_input, x_start = (2 * torch.rand(B, 1, S, S, generator=g) - 1).to(dev), (2 * torch.rand(B, 1, S, S, generator=g) - 1).to(dev)
            ts = []
            for it in range(2 + a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.inner):
                    dt.val_items(pred, target, "l1", x_input, x_start)
                e1.record()
                e1.synchronize()
                if it >= 2:
                    ts.append(e0.elapsed_time(e1) / a.inner)
            med = sorted(ts)[len(ts) // 2]
            nbytes = 4 * (4 * B * npix + 2 * B)
            bound = nbytes / HBM_BPS * 1e3
            emit(dict(leg="b_fd_val_items_f32", batch=B, size=S, ms=round(med, 4), min_ms=round(min(ts), 4), MB=round(nbytes / 1e6, 2),
                      GBps=round(nbytes / med / 1e6, 0), bound_ms_at_6p3TBps=round(bound, 4), bound_over_ms=round(bound / med, 3)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(dict(tool="tools/validate_bench.py", size=S, items=a.items, batch=a.batch, reps=a.reps, inner=a.inner,
                                    rows=rows)) + "\n")


if __name__ == "__main__":
    main()
