"""The fused cross_selective_scan (founddiff_amd.cross_scan_train.cross_scan_fn) against the reference-shaped composition --
oracle.nets.efficient_scan, the x_proj and dt_proj einsums, selective_scan_train.selective_scan_fn, oracle.nets.efficient_merge
and the final transpose -- at the seven training shapes of the reference (train.py: batch 2 from a 512 x 512 slice).  Both end
at y before out_norm.  One JSON line per shape: forward and backward milliseconds of each (median of --reps timed calls after
--warmup; the backward timed from a graph built once and kept, retain_graph) and torch.cuda.max_memory_allocated over one
forward + backward above what the inputs hold.

    python tools/cross_scan_train_bench.py [--batch 2] [--reps 10] [--warmup 2]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (level, image H = W, d_inner, N, R)
SHAPES = [("down0", 512, 128, 4, 4), ("down1", 256, 128, 8, 4), ("down2", 128, 256, 16, 8), ("down3", 64, 512, 32, 16),
          ("mid", 64, 1024, 32, 32), ("ups0", 128, 512, 16, 16), ("ups1", 256, 256, 8, 8)]
PARAMS = ("x_proj_weight", "dt_projs_weight", "dt_projs_bias", "A_logs", "Ds")


def composition(x, p):
    from founddiff_amd.selective_scan_train import selective_scan_fn
    from oracle import nets
    Bn, D, H, W = x.shape
    N = p["A_logs"].shape[1]
    K, _, R = p["dt_projs_weight"].shape
    xs = nets.efficient_scan(x)
    L = xs.shape[-1]
    x_dbl = torch.einsum("bkdl,kcd->bkcl", xs, p["x_proj_weight"])
    dts, Bs, Cs = torch.split(x_dbl, [R, N, N], dim=2)
    dts = torch.einsum("bkrl,kdr->bkdl", dts, p["dt_projs_weight"])
    ys = selective_scan_fn(xs.reshape(Bn, -1, L), dts.contiguous().reshape(Bn, -1, L), -torch.exp(p["A_logs"]),
                           Bs.contiguous(), Cs.contiguous(), p["Ds"], p["dt_projs_bias"].reshape(-1), delta_softplus=True)
    y = nets.efficient_merge(ys.view(Bn, K, -1, L), H, W)
    return y.transpose(1, 2).contiguous().view(Bn, H, W, D)


def fused(x, p):
    from founddiff_amd.cross_scan_train import cross_scan_fn
    return cross_scan_fn(x, *[p[k] for k in PARAMS])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default=",".join(s[0] for s in SHAPES))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    b = a.batch

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        ts = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return sorted(ts)[len(ts) // 2]

    for name, HW, D, N, R in SHAPES:
        if name not in a.shapes.split(","):
            continue
        g = torch.Generator(device=dev).manual_seed(0)
        p = dict(x_proj_weight=torch.randn(4, R + 2 * N, D, device=dev, generator=g) * D ** -0.5,
                 dt_projs_weight=torch.randn(4, D, R, device=dev, generator=g) * R ** -0.5,
                 dt_projs_bias=torch.rand(4, D, device=dev, generator=g) * 4 - 6,
                 A_logs=torch.log(torch.arange(1, N + 1, device=dev).float())[None].repeat(4 * D, 1),
                 Ds=torch.ones(4 * D, device=dev))
        p = {k: v.requires_grad_() for k, v in p.items()}
        x = torch.randn(b, D, HW, HW, device=dev, generator=g).requires_grad_()
        dy = torch.randn(b, HW, HW, D, device=dev, generator=g)
        leaves = [x] + [p[k] for k in PARAMS]
        row = dict(shape=name, batch=b, H=HW, W=HW, d_inner=D, N=N, R=R)
        for tag, fn in (("fused", fused), ("comp", composition)):
            with torch.no_grad():
                t_f = timed(lambda: fn(x, p))
            y = fn(x, p)
            t_b = timed(lambda: torch.autograd.grad(y, leaves, dy, retain_graph=True))
            del y
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            y = fn(x, p)
            torch.autograd.grad(y, leaves, dy)
            del y
            torch.cuda.synchronize()
            row.update({f"{tag}_fwd_ms": round(t_f, 3), f"{tag}_bwd_ms": round(t_b, 3),
                        f"{tag}_peak_MB": round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)})
            torch.cuda.empty_cache()
        row["speedup_fwd_bwd"] = round((row["comp_fwd_ms"] + row["comp_bwd_ms"]) / (row["fused_fwd_ms"] + row["fused_bwd_ms"]), 2)
        row["memory_ratio"] = round(row["fused_peak_MB"] / row["comp_peak_MB"], 3)
        print(json.dumps(row), flush=True)
        del x, dy, p, leaves
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
