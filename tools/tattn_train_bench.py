"""The fused TransposedAttention core (founddiff_amd.tattn_train.tattn_core_fn) against the torch composition of the reference
(src/DADiff.py:266-281): NCHW F.conv2d(groups=3C), chunk, F.normalize, matmul, softmax, matmul -- at the seven training shapes of
the reference (train.py: batch 2 from a 512 x 512 slice).  Both start from the qkv GEMM's output (channel-last, as F.linear
leaves it; the composition pays the reference's permute + contiguous on the way in and out) and end before project_out.  One
JSON line per shape: forward and backward milliseconds of each (median of --reps timed calls after --warmup, the two variants
alternated call by call; the backward timed from a graph built once and kept, retain_graph) and
torch.cuda.max_memory_allocated over one forward + backward above what the inputs hold.

    python tools/tattn_train_bench.py [--batch 2] [--reps 10] [--warmup 2] [--shapes down0,mid]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (level, image H = W, hidden size C)
SHAPES = [("down0", 512, 64), ("down1", 256, 64), ("down2", 128, 128), ("down3", 64, 256), ("mid", 64, 512), ("ups0", 128, 256),
          ("ups1", 256, 128)]
ARGS = ("qkv_pre", "dw_weight", "temperature")


def composition(a):
    x = a["qkv_pre"].permute(0, 3, 1, 2).contiguous()
    B, C3, H, W = x.shape
    heads = C3 // 96
    q, k, v = F.conv2d(x, a["dw_weight"], None, padding=1, groups=C3).chunk(3, dim=1)
    q, k, v = (t.reshape(B, heads, 32, H * W) for t in (q, k, v))
    q, k = F.normalize(q, dim=-1), F.normalize(k, dim=-1)
    attn = ((q @ k.transpose(-2, -1)) * a["temperature"]).softmax(dim=-1)
    return (attn @ v).reshape(B, C3 // 3, H, W).permute(0, 2, 3, 1).contiguous()


def fused(a):
    from founddiff_amd.tattn_train import tattn_core_fn
    return tattn_core_fn(a["qkv_pre"], a["dw_weight"], None, a["temperature"])


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
    for name, HW, C in SHAPES:
        if name not in a.shapes.split(","):
            continue
        g = torch.Generator(device=dev).manual_seed(0)
        rn = lambda *s: torch.randn(*s, device=dev, generator=g)
        p = dict(qkv_pre=rn(b, HW, HW, 3 * C), dw_weight=rn(3 * C, 1, 3, 3) / 3,
                 temperature=0.5 + 3.5 * torch.rand(C // 32, 1, 1, device=dev, generator=g))
        p = {k: v.requires_grad_() for k, v in p.items()}
        dout = rn(b, HW, HW, C)
        leaves = [p[k] for k in ARGS]
        row = dict(shape=name, batch=b, H=HW, W=HW, C=C)
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
