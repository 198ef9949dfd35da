"""The fused SS2D core (founddiff_amd.ss2d_train.ss2d_core_fn) against the best composition a user had before it -- SS2D.forward's
torch glue (chunk, SiLU, permute + contiguous, F.conv2d(groups=D), SiLU, LayerNorm, * z, + local) around
cross_scan_train.cross_selective_scan -- at the seven training shapes of the reference (train.py: batch 2 from a 512 x 512
slice).  Both start from xz (in_proj's output) and end before out_proj.  One JSON line per shape: forward and backward
milliseconds of each (median of --reps timed calls after --warmup, the two variants alternated call by call; the backward timed
from a graph built once and kept, retain_graph) and torch.cuda.max_memory_allocated over one forward + backward above what the
inputs hold.

    python tools/ss2d_train_bench.py [--batch 2] [--reps 10] [--warmup 2] [--shapes down0,mid]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (level, image H = W, d_inner, N, R)
SHAPES = [("down0", 512, 128, 4, 4), ("down1", 256, 128, 8, 4), ("down2", 128, 256, 16, 8), ("down3", 64, 512, 32, 16),
          ("mid", 64, 1024, 32, 32), ("ups0", 128, 512, 16, 16), ("ups1", 256, 256, 8, 8)]
ARGS = ("xz", "conv_weight", "conv_bias", "x_proj_weight", "dt_projs_weight", "dt_projs_bias", "A_logs", "Ds", "norm_weight",
        "norm_bias", "local")


def composition(a):
    from founddiff_amd.cross_scan_train import cross_selective_scan
    D = a["norm_weight"].shape[0]
    x, z = a["xz"].chunk(2, dim=-1)
    z = F.silu(z)
    x = x.permute(0, 3, 1, 2).contiguous()
    x = F.silu(F.conv2d(x, a["conv_weight"], a["conv_bias"], padding=1, groups=D))
    norm = lambda y: F.layer_norm(y, (D,), a["norm_weight"], a["norm_bias"], 1e-5)
    y = cross_selective_scan(x, a["x_proj_weight"], None, a["dt_projs_weight"], a["dt_projs_bias"], a["A_logs"], a["Ds"], norm,
                             nrows=1, delta_softplus=True, step_size=2)
    return y * z + a["local"][:, None, None, :]


def fused(a):
    from founddiff_amd.ss2d_train import ss2d_core_fn
    return ss2d_core_fn(*[a[k] for k in ARGS])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default=",".join(s[0] for s in SHAPES))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    b = a.batch

    def timed(fns):
        """median milliseconds of each callable, alternated call by call"""
        for _ in range(a.warmup):
            for fn in fns:
                fn()
        ts = [[] for _ in fns]
        for _ in range(a.reps):
            for i, fn in enumerate(fns):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ts[i].append(e0.elapsed_time(e1))
        return [sorted(t)[len(t) // 2] for t in ts], [(min(t), max(t)) for t in ts]

    variants = (("fused", fused), ("comp", composition))
    for name, HW, D, N, R in SHAPES:
        if name not in a.shapes.split(","):
            continue
        g = torch.Generator(device=dev).manual_seed(0)
        rn = lambda *s: torch.randn(*s, device=dev, generator=g)
        p = dict(xz=rn(b, HW, HW, 2 * D), conv_weight=rn(D, 1, 3, 3) / 3, conv_bias=0.1 * rn(D),
                 x_proj_weight=rn(4, R + 2 * N, D) * D ** -0.5, dt_projs_weight=rn(4, D, R) * R ** -0.5,
                 dt_projs_bias=torch.rand(4, D, device=dev, generator=g) * 4 - 6,
                 A_logs=torch.log(torch.arange(1, N + 1, device=dev).float())[None].repeat(4 * D, 1),
                 Ds=torch.ones(4 * D, device=dev), norm_weight=1 + 0.1 * rn(D), norm_bias=0.1 * rn(D), local=rn(b, D))
        p = {k: v.requires_grad_() for k, v in p.items()}
        dout = rn(b, HW, HW, D)
        leaves = [p[k] for k in ARGS]
        row = dict(shape=name, batch=b, H=HW, W=HW, d_inner=D, N=N, R=R)
        with torch.no_grad():
            t_f, s_f = timed([lambda fn=fn: fn(p) for _, fn in variants])
        outs = [fn(p) for _, fn in variants]
        t_b, s_b = timed([lambda o=o: torch.autograd.grad(o, leaves, dout, retain_graph=True) for o in outs])
        del outs
        for i, (tag, fn) in enumerate(variants):
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            o = fn(p)
            torch.autograd.grad(o, leaves, dout)
            del o
            torch.cuda.synchronize()
            row.update({f"{tag}_fwd_ms": round(t_f[i], 3), f"{tag}_bwd_ms": round(t_b[i], 3),
                        f"{tag}_fwd_bwd_spread_ms": [round(s_f[i][0] + s_b[i][0], 3), round(s_f[i][1] + s_b[i][1], 3)],
                        f"{tag}_peak_MB": round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)})
            torch.cuda.empty_cache()
        row["speedup_fwd_bwd"] = round((row["comp_fwd_ms"] + row["comp_bwd_ms"]) / (row["fused_fwd_ms"] + row["fused_bwd_ms"]), 2)
        row["memory_ratio"] = round(row["fused_peak_MB"] / row["comp_peak_MB"], 3)
        print(json.dumps(row), flush=True)
        del p, dout, leaves
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
