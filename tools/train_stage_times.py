"""Where the time of one training step goes: one whole train_step of UnetTrunk(64) at batch 2 from a 512 x 512 slice (pred_res / l1,
clip + Adam + EMA), forward and backward milliseconds per stage and level -- init_conv, each Mamba_block, each ResnetBlock, each
resampling convolution, final_conv, q_sample + loss, and the optimiser.

The forward is timed with device events at the stage boundaries.  The backward with Tensor.register_hook: an event when the gradient
of a stage's output arrives and one when the gradient of its input does (a torch.cat or an add between two stages, and whatever
autograd runs between the two hooks, counts with the stage that is waiting; init_conv has no input gradient, its backward ends with
backward()).  The events cost nothing on the device but the hooks run on the host, so the sum of the stages can exceed the
untimed step, which is reported next to it (median of --reps).  One JSON line, also written to profiles/train_stage_times.json.

    python tools/train_stage_times.py [--batch 2] [--size 512] [--reps 5] [--warmup 2] [--torch-outer]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
T = 1000


def stage_names(levels):
    """the calls of unet_trunk_forward in order: (kind, name, resolution level)"""
    out = []
    for i in range(levels):
        out += [("mamba", f"downs.{i}.mamba", i), ("res", f"downs.{i}.res", i), ("resample", f"downs.{i}.resample", i)]
    out += [("res", "mid.res", levels - 1), ("mamba", "mid.mamba", levels - 1)]
    for i in range(levels):
        lv = levels - 1 - i
        out += [("res", f"ups.{i}.res", lv), ("mamba", f"ups.{i}.mamba", lv), ("resample", f"ups.{i}.resample", lv)]
    out.append(("res", "final.res", 0))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--torch-outer", action="store_true", help="init_conv and final_conv through torch, as before outer_conv_train")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_stage_times.json"))
    a = ap.parse_args()
    from founddiff_amd import diffusion_train as dt
    from founddiff_amd import unet_train as ut
    from founddiff_amd.DADiff import residual_schedule
    from founddiff_amd.outer_conv_train import final_conv_fn, init_conv_fn
    dev = torch.device("cuda:0")
    B, S = a.batch, a.size
    g = torch.Generator(device=dev).manual_seed(0)
    sch = residual_schedule(T)
    trunk = ut.UnetTrunk(64).to(dev)
    levels = len(trunk.downs)
    dose = F.normalize(torch.randn(B, 1024, device=dev, generator=g), dim=-1)
    c = F.normalize(torch.randn(B, 1, 256, device=dev, generator=g), dim=-1)
    imgs = [torch.rand(B, 1, S, S, device=dev, generator=g), torch.rand(B, 1, S, S, device=dev, generator=g)]
    t = torch.randint(0, T, (B,), device=dev, generator=g)
    seeds = torch.arange(B, device=dev, dtype=torch.int64) + 11
    opt = dt.ClipAdamEMA(list(trunk.parameters()), lr=1e-4, betas=(0.9, 0.99))
    outer = {} if a.torch_outer else dict(init_fn=init_conv_fn, final_fn=final_conv_fn)

    ev = lambda: torch.cuda.Event(enable_timing=True)
    rec = {}            # name -> [fwd0, fwd1, bwd0, bwd1] events of the current step
    order = []

    def mark(name, slot):
        e = ev()
        e.record()
        rec.setdefault(name, [None] * 4)[slot] = e

    def staged(name, fn, x, *rest):
        mark(name, 0)
        if x.requires_grad:
            x.register_hook(lambda grad, n=name: mark(n, 3))
        out = fn(x, *rest)
        mark(name, 1)
        out.register_hook(lambda grad, n=name: mark(n, 2))
        return out

    real = dict(mamba=ut.mamba_block_forward, res=ut.resnet_block_nhwc, resample=ut.resample_nhwc)

    def patched(kind):
        def call(module, x, *rest):
            k, name, _ = order.pop(0)
            assert k == kind, (k, kind)
            return staged(name, lambda xx, *r: real[kind](module, xx, *r), x, *rest)
        return call

    def init_stage(x, w, b):
        fn = init_conv_fn if not a.torch_outer else (lambda x, w, b: ut._nhwc(F.conv2d(x.contiguous(memory_format=torch.channels_last),
                                                                                        w, b, padding=3)))
        return staged("init_conv", fn, x, w, b)

    def final_stage(x, w, b):
        fn = final_conv_fn if not a.torch_outer else (lambda x, w, b: F.conv2d(x.permute(0, 3, 1, 2), w, b))
        return staged("final_conv", fn, x, w, b)

    def plain_step():
        fn = lambda x, times: [ut.unet_trunk_forward(trunk, x, times[0], dose, c, **outer)]
        dt.train_step(fn, opt, imgs, t=t, slice_seeds=seeds, schedule=sch, objective="pred_res", loss_type="l1")

    def staged_step():
        """train_step's body (p_losses_fn -> backward -> opt.step) with the marks"""
        rec.clear()
        order[:] = stage_names(levels)
        ut.mamba_block_forward, ut.resnet_block_nhwc, ut.resample_nhwc = patched("mamba"), patched("res"), patched("resample")
        try:
            mark("step", 0)
            x_in, x_res, _, times = dt.q_sample(imgs[0], imgs[1], t, sch, slice_seeds=seeds)
            mark("q_sample", 0)
            out = ut.unet_trunk_forward(trunk, x_in, times[0], dose, c, init_fn=init_stage, final_fn=final_stage)
            mark("loss", 0)
            loss = dt.residual_loss(out, x_res, "l1")
            mark("loss", 1)
            loss.backward()
            mark("backward", 1)
            opt.step()
            mark("step", 1)
        finally:
            ut.mamba_block_forward, ut.resnet_block_nhwc, ut.resample_nhwc = real["mamba"], real["res"], real["resample"]
        torch.cuda.synchronize()
        assert not order
        ms = lambda e0, e1: e0.elapsed_time(e1)
        row = {}
        for name, (f0, f1, b0, b1) in rec.items():
            if name in ("step", "q_sample", "loss", "backward"):
                continue
            row[name] = (ms(f0, f1), ms(b0, b1 if b1 is not None else rec["backward"][1]))
        row["q_sample"] = (ms(rec["step"][0], rec["q_sample"][0]), 0.0)
        row["loss"] = (ms(rec["loss"][0], rec["loss"][1]), ms(rec["loss"][1], rec["final_conv"][2]))
        row["optimiser"] = (ms(rec["backward"][1], rec["step"][1]), 0.0)
        row["step"] = (ms(rec["step"][0], rec["step"][1]), 0.0)
        return row

    def wall(fn):
        e0, e1 = ev(), ev()
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(a.warmup):
        plain_step()
        staged_step()
    plain, rows = [], []
    for _ in range(a.reps):                                              # the two alternated
        plain.append(wall(plain_step))
        rows.append(staged_step())
    med = lambda v: sorted(v)[len(v) // 2]
    level = {name: lv for _, name, lv in stage_names(levels)}
    stages = []
    for name in rows[0]:
        if name == "step":
            continue
        stages.append(dict(stage=name, level=level.get(name, 0), fwd_ms=round(med([r[name][0] for r in rows]), 3),
                           bwd_ms=round(med([r[name][1] for r in rows]), 3)))
    by_kind = {}
    for s in stages:
        kind = s["stage"].rsplit(".", 1)[-1]
        k = by_kind.setdefault(kind, [0.0, 0.0])
        k[0] += s["fwd_ms"]
        k[1] += s["bwd_ms"]
    out = dict(tool="train_stage_times", batch=B, H=S, W=S, dim=64, reps=a.reps, device=torch.cuda.get_device_name(0),
               outer="torch" if a.torch_outer else "hip", step_ms=round(med(plain), 3),
               step_spread_ms=[round(min(plain), 3), round(max(plain), 3)],
               staged_step_ms=round(med([r["step"][0] for r in rows]), 3),
               sum_of_stages_ms=round(sum(s["fwd_ms"] + s["bwd_ms"] for s in stages), 3),
               by_kind_ms={k: [round(v[0], 3), round(v[1], 3)] for k, v in by_kind.items()}, stages=stages)
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
