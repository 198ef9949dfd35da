"""The optimiser step of two U-Nets (founddiff_amd.diffusion_train.ClipRAdamEMA, csrc/fd_train_step.hip's fd_opt_radam_ema_f32)
against the torch composition of the reference's Trainer.train for num_unet=2 (src/DADiff.py:1598-1602, 1707-1725), over the
parameters of two UnetTrunk(64), and one whole two-U-Net training step at batch 2 from 512 x 512 slices.  One JSON line per leg:

  b  the optimiser step: ONE ClipRAdamEMA.step() over the parameters of both trunks against clip_grad_norm_(1.0) over both + two
     torch.optim.RAdam(foreach=True).step() + their zero_grad(), on a step without and on a step with the EMA update (torch: one
     lerp_ per parameter, as ema-pytorch does), at a plain step of the rule (step 3) and at a rectified one (step 8).
     Milliseconds, peak MB above what is resident, launches per step (torch.profiler; "not measured" if it gives none), and the
     update kernel alone: its bytes (8 x 4 bytes per parameter, 10 x 4 with the EMA) over its time, as a fraction of 6.3 TB/s.
     The kernel moves the Adam kernel's bytes, which reached 0.80 of that bound (profiles/train_step_bench.json): the figure to
     report against.
  c  one whole train_step of both trunks ('pred_res_noise': one q_sample, two forwards and backwards, one optimiser step)
     against two one-U-Net train_steps ('pred_res' on the first trunk, 'pred_noise' on the second, a ClipRAdamEMA each).

Milliseconds are medians of --reps timed calls after --warmup, the two sides alternated call by call in one process; peak MB is
max_memory_allocated above the level before the call.  The baseline lives here, not in the package.

    python tools/radam_step_bench.py [--batch 2] [--size 512] [--reps 10] [--warmup 2] [--legs b,c] [--out profiles/radam_step_bench.json]
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
HBM_BPS = 6.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--legs", default="b,c")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "radam_step_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    from founddiff_amd import _lib as L, diffusion_train as dt
    from founddiff_amd._train import ptr, stream
    from founddiff_amd.DADiff import residual_schedule
    from founddiff_amd.unet_train import UnetTrunk
    B, S = a.batch, a.size
    sch = residual_schedule(T)
    g = torch.Generator(device=dev).manual_seed(0)
    rows = []

    def timed(fns, before=None):
        """median milliseconds of each callable, alternated call by call; before[i] runs untimed ahead of fns[i]"""
        ts = [[] for _ in fns]
        for it in range(a.warmup + a.reps):
            for i, fn in enumerate(fns):
                if before:
                    before[i]()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if it >= a.warmup:
                    ts[i].append(e0.elapsed_time(e1))
        return [sorted(v)[len(v) // 2] for v in ts]

    def peak(fn, before=None):
        if before:
            before()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)

    def launches(fn, before=None):
        """device kernels and copies of one call, or "not measured\""""
        try:
            from torch.profiler import ProfilerActivity, profile
            if before:
                before()
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                fn()
                torch.cuda.synchronize()
            n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
            return n if n > 0 else "not measured"
        except Exception:
            return "not measured"

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    legs = a.legs.split(",")
    torch.manual_seed(0)
    trunks = [UnetTrunk(64).to(dev), UnetTrunk(64).to(dev)]
    # ---- b: the optimiser
    if "b" in legs:
        src = [p for m in trunks for p in m.parameters()]
        n0 = len(list(trunks[0].parameters()))
        pf = [torch.nn.Parameter(p.detach().clone()) for p in src]
        pt = [torch.nn.Parameter(p.detach().clone()) for p in src]
        ef, et = [p.detach().clone() for p in pf], [p.detach().clone() for p in pt]
        g0 = [1e-3 * torch.randn(p.shape, device=dev, generator=g) for p in pf]
        n_elem = sum(p.numel() for p in pf)
        opt_f = dt.ClipRAdamEMA(pf, ef, lr=1e-4)
        opts_t = [torch.optim.RAdam(pt[:n0], lr=1e-4, weight_decay=0.0, foreach=True),
                  torch.optim.RAdam(pt[n0:], lr=1e-4, weight_decay=0.0, foreach=True)]
        for p, gr in zip(pf, g0):
            p.grad = gr.clone()

        def fill_f():
            torch._foreach_copy_([p.grad for p in pf], g0)

        def fill_t():
            for p, gr in zip(pt, g0):
                p.grad = gr.clone()

        def step_f(mode, decay=None):
            return lambda: opt_f.step(ema_mode=mode, ema_decay=decay)

        def step_t(ema):
            def fn():
                torch.nn.utils.clip_grad_norm_(pt, 1.0)
                for o in opts_t:
                    o.step()
                    o.zero_grad()
                if ema:
                    for e, p in zip(et, pt):
                        e.lerp_(p.detach(), 1 - 0.995)
            return fn
        for tag, f_fn, t_fn in (("b_optimiser_step", step_f(0), step_t(False)), ("b_optimiser_step_with_ema", step_f(2, 0.995), step_t(True))):
            ms = timed([f_fn, t_fn], before=[fill_f, fill_t])
            row = dict(leg=tag, tensors=len(pf), elements=n_elem, small_tensors=sum(p.numel() < 4096 for p in pf),
                       fused_ms=round(ms[0], 4), torch_ms=round(ms[1], 4), fused_peak_MB=peak(f_fn, fill_f), torch_peak_MB=peak(t_fn, fill_t),
                       fused_launches=launches(f_fn, fill_f), torch_launches=launches(t_fn, fill_t), steps_after=opt_f.steps()[0])
            row["speedup"] = round(ms[1] / ms[0], 2)
            emit(row)
        # the update kernel alone, at a plain step of the rule and at a rectified one (the step counts are set, not run up to)
        fill_f()
        st = stream(dev)
        for step in (3, 8):
            opt_f._steps.fill_(step)
            rect = dt.radam_scalars(step, 1e-4, 0.9, 0.999)[0]
            for tag, mode, nbytes in (("update", 0, 8 * 4 * n_elem), ("update_with_ema", 2, 10 * 4 * n_elem)):
                k_fn = lambda mode=mode: L.call("fd_opt_radam_ema_f32", ptr(opt_f._chunks), ptr(opt_f._table), ptr(opt_f._steps),
                                                ptr(opt_f._rec), opt_f.nchunk, 1e-4, 0.9, 0.999, 1e-8, mode, 0.995, 1, 0, st)
                ms = timed([k_fn])[0]
                emit(dict(leg=f"b_kernel_{tag}", step=step, rectified=rect, ms=round(ms, 4), MB=round(nbytes / 1e6, 1),
                          GBps=round(nbytes / ms / 1e6, 0), fraction_of_6300_GBps=round(nbytes / (ms * 1e-3) / HBM_BPS, 3)))
        del pf, pt, ef, et, g0, opt_f, opts_t
        torch.cuda.empty_cache()
    # ---- c: a whole step
    if "c" in legs:
        import copy
        imgs = [torch.rand(B, 1, S, S, device=dev, generator=g), torch.rand(B, 1, S, S, device=dev, generator=g)]
        t = torch.randint(0, T, (B,), device=dev, generator=g)
        seeds = torch.arange(B, device=dev, dtype=torch.int64) + 7
        twins = [copy.deepcopy(m) for m in trunks]
        dose = F.normalize(torch.randn(B, 1024, device=dev, generator=g), dim=-1)
        c = F.normalize(torch.randn(B, 1, 256, device=dev, generator=g), dim=-1)
        opt_two = dt.ClipRAdamEMA([p for m in trunks for p in m.parameters()], lr=1e-4)
        opt_one = [dt.ClipRAdamEMA(m.parameters(), lr=1e-4) for m in twins]
        fn_two = lambda x, times: [trunks[0](x, times[0], dose, c), trunks[1](x, times[1], dose, c)]
        fn_one = [lambda x, times: [twins[0](x, times[0], dose, c)], lambda x, times: [twins[1](x, times[1], dose, c)]]

        def two_c():
            dt.train_step(fn_two, opt_two, imgs, t=t, slice_seeds=seeds, schedule=sch, objective="pred_res_noise", loss_type="l1")

        def ones_c():
            for fn, opt, objective in zip(fn_one, opt_one, ("pred_res", "pred_noise")):
                dt.train_step(fn, opt, imgs, t=t, slice_seeds=seeds, schedule=sch, objective=objective, loss_type="l1")
        ms = timed([two_c, ones_c])
        row = dict(leg="c_train_step_two_unets", batch=B, size=S, two_unet_step_ms=round(ms[0], 3), two_one_unet_steps_ms=round(ms[1], 3),
                   two_unet_step_peak_MB=peak(two_c), two_one_unet_steps_peak_MB=peak(ones_c))
        row["ratio"] = round(ms[0] / ms[1], 3)
        emit(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(tool="tools/radam_step_bench.py", batch=B, size=S, reps=a.reps, warmup=a.warmup, rows=rows), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
