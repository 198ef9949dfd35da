"""The structural loss term (diffusion_train.structural_loss, csrc/fd_ssim_train.hip): what it costs and how exact it is.
Everything is reported, nothing is gated.  One JSON line per row, and all of them as one line in --out:

  a  fd_ssim_loss_f32 (structural_loss's forward, which makes the gradient too: pass 1, pass 2, two small sums, the workspace)
     at batch 2 and 8, 512^2 and 256^2, both row kinds, alternated in the same loop with the torch fp32 composition
     (F.pad(reflect) + two conv2d + autograd, forward and backward): milliseconds per call from device events around --inner
     back-to-back calls, median of --reps; the kernel's bytes (pass 1 reads the 2 or 3 images and writes 3 maps, pass 2 reads
     all of them again and writes the gradient), GB/s and those bytes over 6.3 TB/s; torch's launches per call
     (torch.profiler) and the peak memory either holds above the inputs.
  e  the kernel's errors against the float64 composition on the tests' shapes and inputs (tests/ssim_loss_ref.py), beside those
     of the float32 composition on the CPU, whose worst case x 4 is the tests' gate.
  c  a training step at batch 2, 512^2, dim 64 -- diffusion_train.train_step around unet_train.UnetTrunk(64), the step
     tools/train_stage_times.py times (profiles/train_stage_times.json) -- with ssim_weight 0 against 0.5 in alternated blocks
     of --steps steps: per weight the median block and the spread (max - min) of its blocks, milliseconds per step.

    python tools/ssim_loss_bench.py [--reps 5] [--inner 20] [--blocks 5] [--steps 5] [--legs a,e,c] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_BPS = 6.3e12
T = 1000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--legs", default="a,e,c")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ssim_loss_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/ssim_loss_bench.py measures on the GPU: none is visible")
    dev = torch.device("cuda:0")
    import ssim_loss_ref as R
    from founddiff_amd import diffusion_train as dt
    rows, legs = [], a.legs.split(",")
    med = lambda v: sorted(v)[len(v) // 2]

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    def peak_above(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        return (torch.cuda.max_memory_allocated() - base) / 1e6

    if "a" in legs:
        for S in (512, 256):
            for B in (2, 8):
                for residual in (True, False):
                    g = torch.Generator().manual_seed(B + S)
                    x_start, x_input = ((2 * torch.rand(B, 1, S, S, generator=g) - 1).to(dev) for _ in range(2))
                    out = (0.3 * torch.randn(B, 1, S, S, generator=g)).to(dev).requires_grad_(True)
                    xi = x_input if residual else None

                    def hip():
                        dt.structural_loss(out, x_start, xi, residual=residual)           # the gradient is made in the forward

                    def composed():
                        o = out.detach().requires_grad_(True)
                        p, y = R.images(o, x_start, xi, residual)
                        term = 1 - R.ssim_map(p, y).mean(dim=(1, 2, 3)).mean()
                        torch.autograd.grad(term, o)

                    t_hip, t_torch = [], []
                    for it in range(2 + a.reps):                                          # alternated; two untimed rounds first
                        h, c = timed(hip, a.inner), timed(composed, a.inner)
                        if it >= 2:
                            t_hip.append(h), t_torch.append(c)
                    try:
                        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
                            composed()
                            torch.cuda.synchronize()
                        launches = int(sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA))
                    except Exception as err:                                              # a build of torch without the device tracer
                        print(f"torch.profiler: {err!r}: torch_launches is not reported", file=sys.stderr)
                        launches = None
                    nimg = 3 if residual else 2
                    nbytes = 4 * B * S * S * (nimg + 3 + nimg + 3 + 1)
                    bound = nbytes / HBM_BPS * 1e3
                    emit(dict(leg="a_fd_ssim_loss_f32", batch=B, size=S, row="res" if residual else "x0", ms=round(med(t_hip), 4),
                              min_ms=round(min(t_hip), 4), MB=round(nbytes / 1e6, 2), GBps=round(nbytes / med(t_hip) / 1e6, 0),
                              bound_ms_at_6p3TBps=round(bound, 4), bound_over_ms=round(bound / med(t_hip), 3),
                              peak_extra_MB=round(peak_above(hip), 2), torch_ms=round(med(t_torch), 4), torch_min_ms=round(min(t_torch), 4),
                              torch_launches=launches, torch_peak_extra_MB=round(peak_above(composed), 2),
                              torch_over_hip=round(med(t_torch) / med(t_hip), 2)))
    if "e" in legs:
        gv, gi, gg = R.gates()
        worst = dict(value=0.0, items=0.0, grad=0.0)
        for shape in R.SHAPES:
            for residual in (True, False):
                inp, (t64, i64, g64), (t32, i32, g32) = R.case(shape, residual)
                o, x0, xi = (None if v is None else v.to(dev) for v in inp)
                o.requires_grad_(True)
                term = dt.structural_loss(o, x0, xi, residual=residual)
                term.backward()
                items = dt.ssim_items(o, x0, xi, residual=residual).cpu()
                ev, ei = abs(float(term.detach()) - float(t64)), float((items.double() - i64).abs().max())
                eg = R.grad_err(o.grad.cpu(), g64)
                worst = dict(value=max(worst["value"], ev), items=max(worst["items"], ei), grad=max(worst["grad"], eg))
                emit(dict(leg="e_errors", shape=list(shape), row="res" if residual else "x0", value_err=ev, items_err=ei, grad_err=eg,
                          f32_composition_value_err=abs(float(t32) - float(t64)), f32_composition_grad_err=R.grad_err(g32, g64)))
        emit(dict(leg="e_worst", kernel=worst, gate=dict(value=gv, items=gi, grad=gg)))
    if "c" in legs:
        from founddiff_amd import unet_train as ut
        from founddiff_amd.DADiff import residual_schedule
        from founddiff_amd.outer_conv_train import final_conv_fn, init_conv_fn
        B, S = 2, 512
        g = torch.Generator(device=dev).manual_seed(0)
        sch = residual_schedule(T)
        trunk = ut.UnetTrunk(64).to(dev)
        dose = F.normalize(torch.randn(B, 1024, device=dev, generator=g), dim=-1)
        c = F.normalize(torch.randn(B, 1, 256, device=dev, generator=g), dim=-1)
        imgs = [torch.rand(B, 1, S, S, device=dev, generator=g), torch.rand(B, 1, S, S, device=dev, generator=g)]
        t = torch.randint(0, T, (B,), device=dev, generator=g)
        seeds = torch.arange(B, device=dev, dtype=torch.int64) + 11
        opt = dt.ClipAdamEMA(list(trunk.parameters()), lr=1e-4, betas=(0.9, 0.99))
        fn = lambda x, times: [ut.unet_trunk_forward(trunk, x, times[0], dose, c, init_fn=init_conv_fn, final_fn=final_conv_fn)]

        def step(w):
            dt.train_step(fn, opt, imgs, t=t, slice_seeds=seeds, schedule=sch, objective="pred_res", loss_type="l1", ssim_weight=w)

        ms = {0.0: [], 0.5: []}
        for it in range(1 + a.blocks):                                                    # alternated blocks; one untimed round
            for w in (0.0, 0.5):
                v = timed(lambda: step(w), a.steps)
                if it:
                    ms[w].append(v)
        row = dict(leg="c_train_step", batch=B, size=S, dim=64, blocks=a.blocks, steps_per_block=a.steps)
        for w, tag in ((0.0, "w0"), (0.5, "w0p5")):
            row.update({f"{tag}_ms": round(med(ms[w]), 3), f"{tag}_min_ms": round(min(ms[w]), 3),
                        f"{tag}_spread_ms": round(max(ms[w]) - min(ms[w]), 3)})
        row["difference_ms"] = round(med(ms[0.5]) - med(ms[0.0]), 3)
        emit(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(dict(tool="tools/ssim_loss_bench.py", reps=a.reps, inner=a.inner, blocks=a.blocks, steps=a.steps, rows=rows)) + "\n")


if __name__ == "__main__":
    main()
