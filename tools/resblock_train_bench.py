"""The fused ResnetBlock core (founddiff_amd.resblock_train.block_core_fn) against the torch composition the reference runs
(src/DADiff.py:139-154, 213-229, 430): NCHW-contiguous F.conv2d, F.group_norm, F.silu, + res -- at the ten ResnetBlocks of a
forward (train.py: batch 2 from a 512 x 512 slice).  Each side runs in its own layout (channel-last against NCHW) on the same
values; the weight is already standardised on both; blocks with Cin != Cout get a precomputed res, the others res = x.  One JSON
line per shape: forward and backward milliseconds of each (median of --reps timed calls after --warmup, the two variants
alternated call by call; the backward timed from a graph built once and kept, retain_graph), torch.cuda.max_memory_allocated over
one forward + backward above what the inputs hold, and the achieved TFLOP/s of the fd_conv3x3_wgrad_f32 launch alone (2 B H W
9 Cin Cout FLOP; the exact-f32 MFMA's measured ceiling is 155 TFLOP/s).

    python tools/resblock_train_bench.py [--batch 2] [--reps 10] [--warmup 2] [--shapes down0,mid]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (level, image H = W, Cin, Cout)
SHAPES = [("down0", 512, 64, 64), ("down1", 256, 64, 64), ("down2", 128, 128, 128), ("down3", 64, 256, 256), ("mid", 64, 512, 512),
          ("ups0", 64, 768, 512), ("ups1", 128, 384, 256), ("ups2", 256, 192, 128), ("ups3", 512, 128, 64), ("final", 512, 128, 64)]
ARGS = ("x", "weight", "bias", "gn_weight", "gn_bias", "res")


def composition(a):
    h = F.conv2d(a["x"], a["weight"], a["bias"], padding=1)
    return F.silu(F.group_norm(h, 8, a["gn_weight"], a["gn_bias"], 1e-5)) + a.get("res", a["x"])


def fused(a):
    from founddiff_amd.resblock_train import block_core_fn
    return block_core_fn(a["x"], a["weight"], a["bias"], a["gn_weight"], a["gn_bias"], a.get("res", a["x"]))


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

    def wgrad_tflops(HW, cin, cout, g):
        from founddiff_amd import _lib as L
        x, dh = torch.randn(b, HW, HW, cin, device=dev, generator=g), torch.randn(b, HW, HW, cout, device=dev, generator=g)
        dw = torch.empty(cout, 9 * cin, device=dev)
        ws = torch.empty(max(4, int(L.lib().fd_conv3x3_wgrad_ws_floats(b, HW, HW, cin, cout))), device=dev)
        st = torch.cuda.current_stream().cuda_stream
        run = lambda: L.call("fd_conv3x3_wgrad_f32", x.data_ptr(), cin, 0, dh.data_ptr(), dw.data_ptr(), ws.data_ptr(), b, HW, HW,
                             cin, cout, st)
        (ms,), ((lo, hi),) = timed([run])
        flop = 2.0 * b * HW * HW * 9 * cin * cout
        return ms, (lo, hi), flop / (ms * 1e-3) / 1e12

    variants = (("fused", fused), ("comp", composition))
    for name, HW, cin, cout in SHAPES:
        if name not in a.shapes.split(","):
            continue
        g = torch.Generator(device=dev).manual_seed(0)
        rn = lambda *s: torch.randn(*s, device=dev, generator=g)
        p = dict(x=rn(b, HW, HW, cin), weight=rn(cout, cin, 3, 3) / (9 * cin) ** 0.5, bias=0.1 * rn(cout), gn_weight=1 + 0.3 * rn(cout),
                 gn_bias=0.3 * rn(cout))
        if cin != cout:
            p["res"] = rn(b, HW, HW, cout)
        # the composition's copies: the same values NCHW-contiguous
        q = {k: (v.permute(0, 3, 1, 2).contiguous() if k in ("x", "res") else v.clone()) for k, v in p.items()}
        sides = [{k: v.requires_grad_() for k, v in d.items()} for d in (p, q)]
        dout = rn(b, HW, HW, cout)
        douts = [dout, dout.permute(0, 3, 1, 2).contiguous()]
        leaves = [[d[k] for k in ARGS if k in d] for d in sides]
        row = dict(shape=name, batch=b, H=HW, W=HW, Cin=cin, Cout=cout)
        with torch.no_grad():
            t_f, s_f = timed([lambda fn=fn, d=d: fn(d) for (_, fn), d in zip(variants, sides)])
        outs = [fn(d) for (_, fn), d in zip(variants, sides)]
        t_b, s_b = timed([lambda o=o, lv=lv, do=do: torch.autograd.grad(o, lv, do, retain_graph=True)
                          for o, lv, do in zip(outs, leaves, douts)])
        del outs
        for i, (tag, fn) in enumerate(variants):
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            o = fn(sides[i])
            torch.autograd.grad(o, leaves[i], douts[i])
            del o
            torch.cuda.synchronize()
            row.update({f"{tag}_fwd_ms": round(t_f[i], 3), f"{tag}_bwd_ms": round(t_b[i], 3),
                        f"{tag}_fwd_bwd_spread_ms": [round(s_f[i][0] + s_b[i][0], 3), round(s_f[i][1] + s_b[i][1], 3)],
                        f"{tag}_peak_MB": round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)})
            torch.cuda.empty_cache()
        row["speedup_fwd_bwd"] = round((row["comp_fwd_ms"] + row["comp_bwd_ms"]) / (row["fused_fwd_ms"] + row["fused_bwd_ms"]), 2)
        row["memory_ratio"] = round(row["fused_peak_MB"] / row["comp_peak_MB"], 3)
        del p, q, sides, dout, douts, leaves
        torch.cuda.empty_cache()
        ms, (lo, hi), tf = wgrad_tflops(HW, cin, cout, g)
        row.update(wgrad_ms=round(ms, 3), wgrad_spread_ms=[round(lo, 3), round(hi, 3)], wgrad_TFLOPs=round(tf, 1),
                   wgrad_fraction_of_155=round(tf / 155.0, 3))
        print(json.dumps(row), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
