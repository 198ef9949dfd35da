"""The training step (founddiff_amd.diffusion_train, csrc/fd_train_step.hip) against the torch composition of the reference's
Trainer.train (src/DADiff.py:1382-1499, 1689-1725), at batch 2 from a 512 x 512 slice with UnetTrunk(64).  One JSON line per leg:

  a  q_sample + loss, forward and backward: q_sample (keyed noise) + residual_loss + backward against the torch lines of
     ResidualDiffusion.forward / p_losses (normalize, randn_like, x_res, q_sample, cat, the two time inputs, l1_loss -> mean) +
     backward, on a leaf tensor in the U-Net's place.
  b  the optimiser step over the trunk's parameters: ClipAdamEMA.step() against clip_grad_norm_(1.0) +
     torch.optim.Adam(foreach=True).step() + zero_grad(), on a step without and on a step with the EMA update (torch: one lerp_
     per parameter, as ema-pytorch does).  Milliseconds, peak MB above what is resident, launches per step (torch.profiler; "not
     measured" if the profiler gives none), and the update kernel alone: its bytes (8 x 4 bytes per parameter) over its time,
     as a fraction of 6.3 TB/s.
  c  one whole train_step of the trunk against the same trunk driven by the torch lines of a and b, and the share of the step that
     a + b are on each side.

Milliseconds are medians of --reps timed calls after --warmup, the two sides alternated call by call in one process; peak MB is
max_memory_allocated above the level before the call.  The baseline lives here, not in the package.

    python tools/train_step_bench.py [--batch 2] [--size 512] [--reps 10] [--warmup 2] [--legs a,b,c] [--out FILE]
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


def torch_p_losses(model_fn, imgs, t, acs, bcs, loss_type="l1"):
    """ResidualDiffusion.forward + p_losses, pred_res, condition=True (src/DADiff.py:1399-1499)"""
    x_start, x_input = imgs[0] * 2 - 1, imgs[1] * 2 - 1
    noise = torch.randn_like(x_start)
    x_res = x_input - x_start
    x = x_start + acs[t].view(-1, 1, 1, 1) * x_res + bcs[t].view(-1, 1, 1, 1) * noise
    x_in = torch.cat((x, x_input), dim=1)
    out = model_fn(x_in, [acs[t] * T, bcs[t] * T])
    loss = (F.l1_loss if loss_type == "l1" else F.mse_loss)(out[0], x_res, reduction="none")
    return [loss.flatten(1).mean(dim=1).mean()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--legs", default="a,b,c")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    from founddiff_amd import _lib as L, diffusion_train as dt
    from founddiff_amd._train import ptr, stream
    from founddiff_amd.DADiff import residual_schedule
    from founddiff_amd.unet_train import UnetTrunk
    B, S = a.batch, a.size
    sch = residual_schedule(T)
    acs, bcs = sch["alphas_cumsum"].to(dev), sch["betas_cumsum"].to(dev)
    g = torch.Generator(device=dev).manual_seed(0)
    imgs = [torch.rand(B, 1, S, S, device=dev, generator=g), torch.rand(B, 1, S, S, device=dev, generator=g)]
    t = torch.randint(0, T, (B,), device=dev, generator=g)
    seeds = torch.arange(B, device=dev, dtype=torch.int64) + 7
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
    ms_ab = {}
    # ---- a: q_sample + loss
    if "a" in legs:
        pred = torch.randn(B, 1, S, S, device=dev, generator=g).requires_grad_()
        leaf_fn = lambda x_in, times: [pred]

        def fused_a():
            pred.grad = None
            for loss in dt.p_losses_fn(leaf_fn, imgs, t, sch, "pred_res", "l1", slice_seeds=seeds, normalize=True):
                loss.backward()

        def torch_a():
            pred.grad = None
            for loss in torch_p_losses(leaf_fn, imgs, t, acs, bcs):
                loss.backward()
        ms = timed([fused_a, torch_a])
        row = dict(leg="a_qsample_loss_fwd_bwd", batch=B, size=S, fused_ms=round(ms[0], 4), torch_ms=round(ms[1], 4),
                   fused_peak_MB=peak(fused_a), torch_peak_MB=peak(torch_a), fused_launches=launches(fused_a),
                   torch_launches=launches(torch_a))
        row["speedup"] = round(ms[1] / ms[0], 2)
        ms_ab["a"] = ms
        emit(row)
        del pred
    # ---- b: the optimiser
    if "b" in legs or "c" in legs:
        torch.manual_seed(0)
        trunk = UnetTrunk(64).to(dev)
    if "b" in legs:
        import copy
        pf = [torch.nn.Parameter(p.detach().clone()) for p in trunk.parameters()]
        pt = [torch.nn.Parameter(p.detach().clone()) for p in trunk.parameters()]
        ef, et = [p.detach().clone() for p in pf], [p.detach().clone() for p in pt]
        g0 = [1e-3 * torch.randn(p.shape, device=dev, generator=g) for p in pf]
        n_elem = sum(p.numel() for p in pf)
        opt_f = dt.ClipAdamEMA(pf, ef, lr=1e-4, betas=(0.9, 0.99))
        opt_t = torch.optim.Adam(pt, lr=1e-4, betas=(0.9, 0.99), foreach=True)
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
                opt_t.step()
                opt_t.zero_grad()
                if ema:
                    for e, p in zip(et, pt):
                        e.lerp_(p.detach(), 1 - 0.995)
            return fn
        for tag, f_fn, t_fn in (("b_optimiser_step", step_f(0), step_t(False)), ("b_optimiser_step_with_ema", step_f(2, 0.995), step_t(True))):
            ms = timed([f_fn, t_fn], before=[fill_f, fill_t])
            row = dict(leg=tag, tensors=len(pf), elements=n_elem, small_tensors=sum(p.numel() < 4096 for p in pf),
                       fused_ms=round(ms[0], 4), torch_ms=round(ms[1], 4), fused_peak_MB=peak(f_fn, fill_f), torch_peak_MB=peak(t_fn, fill_t),
                       fused_launches=launches(f_fn, fill_f), torch_launches=launches(t_fn, fill_t))
            row["speedup"] = round(ms[1] / ms[0], 2)
            ms_ab.setdefault("b", ms)
            emit(row)
        # the update kernel alone
        fill_f()
        st = stream(dev)
        for tag, mode, nbytes in (("update", 0, 8 * 4 * n_elem), ("update_with_ema", 2, 10 * 4 * n_elem)):
            k_fn = lambda mode=mode: L.call("fd_opt_adam_ema_f32", ptr(opt_f._chunks), ptr(opt_f._table), ptr(opt_f._steps),
                                            ptr(opt_f._rec), opt_f.nchunk, 1e-4, 0.9, 0.99, 1e-8, mode, 0.995, 1, 0, st)
            ms = timed([k_fn])[0]
            emit(dict(leg=f"b_kernel_{tag}", ms=round(ms, 4), MB=round(nbytes / 1e6, 1), GBps=round(nbytes / ms / 1e6, 0),
                      fraction_of_6300_GBps=round(nbytes / (ms * 1e-3) / HBM_BPS, 3)))
        del pf, pt, ef, et, g0, opt_f, opt_t
        torch.cuda.empty_cache()
    # ---- c: a whole step
    if "c" in legs:
        import copy
        twin = copy.deepcopy(trunk)
        dose = F.normalize(torch.randn(B, 1024, device=dev, generator=g), dim=-1)
        c = F.normalize(torch.randn(B, 1, 256, device=dev, generator=g), dim=-1)
        opt_f = dt.ClipAdamEMA(trunk.parameters(), lr=1e-4, betas=(0.9, 0.99))
        opt_t = torch.optim.Adam(twin.parameters(), lr=1e-4, betas=(0.9, 0.99), foreach=True)
        fn_f = lambda x, times: [trunk(x, times[0], dose, c)]
        fn_t = lambda x, times: [twin(x, times[0], dose, c)]

        def fused_c():
            dt.train_step(fn_f, opt_f, imgs, t=t, slice_seeds=seeds, schedule=sch, objective="pred_res", loss_type="l1")

        def torch_c():
            for loss in torch_p_losses(fn_t, imgs, t, acs, bcs):
                loss.backward()
            torch.nn.utils.clip_grad_norm_(twin.parameters(), 1.0)
            opt_t.step()
            opt_t.zero_grad()
        ms = timed([fused_c, torch_c])
        row = dict(leg="c_train_step", batch=B, size=S, fused_ms=round(ms[0], 3), torch_ms=round(ms[1], 3),
                   fused_peak_MB=peak(fused_c), torch_peak_MB=peak(torch_c))
        row["speedup"] = round(ms[1] / ms[0], 3)
        if "a" in ms_ab and "b" in ms_ab:
            row["fused_share_of_a_plus_b"] = round((ms_ab["a"][0] + ms_ab["b"][0]) / ms[0], 4)
            row["torch_share_of_a_plus_b"] = round((ms_ab["a"][1] + ms_ab["b"][1]) / ms[1], 4)
        else:
            row["fused_share_of_a_plus_b"] = row["torch_share_of_a_plus_b"] = "not measured"
        emit(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(tool="tools/train_step_bench.py", batch=B, size=S, reps=a.reps, warmup=a.warmup, rows=rows), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
