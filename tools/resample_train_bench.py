"""The eight resampling / level-end convolutions of the U-Net through founddiff_amd.resample_train (downsample_fn, upsample_fn,
conv3x3_fn) against the torch composition (F.conv2d(stride 2) / F.interpolate + F.conv2d / F.conv2d, fp32 on channels-last
memory) at the training shapes (train.py: batch 2 from a 512 x 512 slice; the levels of tools/resblock_train_bench.py).  Both sides
run in the same process on the same values.  One JSON line per convolution: forward and backward milliseconds of each (median of
--reps timed calls after --warmup, the two variants alternated call by call; the backward timed from a graph built once and kept,
retain_graph), torch.cuda.max_memory_allocated over one forward + backward above what the inputs hold, and the achieved TFLOP/s
of the fd_conv_sub2x_f32 and fd_corr4x4s2_f32 launches alone (2 x 16 Cin Cout FLOP per source / coarse pixel; the exact-f32 MFMA's
measured ceiling is 155 TFLOP/s).

    python tools/resample_train_bench.py [--batch 2] [--reps 10] [--warmup 2] [--shapes down0,up2]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (name, kind, input H = W, Cin, Cout)
SHAPES = [("down0", "down", 512, 64, 64), ("down1", "down", 256, 64, 128), ("down2", "down", 128, 128, 256),
          ("down3", "conv3", 64, 256, 512), ("up0", "up", 64, 512, 256), ("up1", "up", 128, 256, 128), ("up2", "up", 256, 128, 64),
          ("up3", "conv3", 512, 64, 64)]
ARGS = ("x", "weight", "bias")


def composition(kind, a):
    if kind == "down":
        return F.conv2d(a["x"], a["weight"], a["bias"], stride=2, padding=1)
    x = F.interpolate(a["x"], scale_factor=2, mode="nearest") if kind == "up" else a["x"]
    return F.conv2d(x, a["weight"], a["bias"], padding=1)


def fused(kind, a):
    from founddiff_amd import resample_train as rt
    return dict(down=rt.downsample_fn, up=rt.upsample_fn, conv3=rt.conv3x3_fn)[kind](a["x"], a["weight"], a["bias"])


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

    def kernel_tflops(HW, cs, cc, g):
        """the two new kernels alone on a source / coarse grid of HW x HW: sub2x cs -> cc, corr with P = cs, Q = cc"""
        from founddiff_amd import _lib as L
        st = torch.cuda.current_stream().cuda_stream
        x, w2 = torch.randn(b, HW, HW, cs, device=dev, generator=g), torch.randn(cc, 16 * cs, device=dev, generator=g)
        out = torch.empty(b, 2 * HW, 2 * HW, cc, device=dev)
        run = lambda: L.call("fd_conv_sub2x_f32", x.data_ptr(), w2.data_ptr(), None, out.data_ptr(), b, HW, HW, cs, cc, st)
        (ms1,), ((lo1, hi1),) = timed([run])
        del w2
        gbuf = torch.empty(cs, 16 * cc, device=dev)
        ws = torch.empty(max(4, int(L.lib().fd_corr4x4s2_ws_floats(b, HW, HW, cs, cc))), device=dev)
        fine = out.normal_(generator=g)
        run = lambda: L.call("fd_corr4x4s2_f32", x.data_ptr(), fine.data_ptr(), gbuf.data_ptr(), ws.data_ptr(), b, HW, HW, cs, cc,
                             st)
        (ms2,), ((lo2, hi2),) = timed([run])
        flop = 2.0 * b * HW * HW * 16 * cs * cc
        return dict(sub2x_ms=round(ms1, 3), sub2x_spread_ms=[round(lo1, 3), round(hi1, 3)],
                    sub2x_TFLOPs=round(flop / (ms1 * 1e-3) / 1e12, 1), corr_ms=round(ms2, 3),
                    corr_spread_ms=[round(lo2, 3), round(hi2, 3)], corr_TFLOPs=round(flop / (ms2 * 1e-3) / 1e12, 1))

    for name, kind, HW, cin, cout in SHAPES:
        if name not in a.shapes.split(","):
            continue
        g = torch.Generator(device=dev).manual_seed(0)
        rn = lambda *s: torch.randn(*s, device=dev, generator=g)
        k = 4 if kind == "down" else 3
        OH = dict(down=HW // 2, up=2 * HW, conv3=HW)[kind]
        p = dict(x=rn(b, HW, HW, cin), weight=rn(cout, cin, k, k) / (k * k * cin) ** 0.5, bias=0.1 * rn(cout))
        # the composition's copies: the same values, NCHW shapes on channels-last memory
        q = dict(x=p["x"].clone().permute(0, 3, 1, 2), weight=p["weight"].clone().contiguous(memory_format=torch.channels_last),
                 bias=p["bias"].clone())
        sides = [{k_: v.requires_grad_() for k_, v in d.items()} for d in (p, q)]
        dout = rn(b, OH, OH, cout)
        douts = [dout, dout.clone().permute(0, 3, 1, 2)]
        leaves = [[d[k_] for k_ in ARGS] for d in sides]
        variants = (("fused", fused), ("comp", composition))
        row = dict(shape=name, kind=kind, batch=b, H=HW, W=HW, Cin=cin, Cout=cout)
        with torch.no_grad():
            t_f, s_f = timed([lambda fn=fn, d=d: fn(kind, d) for (_, fn), d in zip(variants, sides)])
        outs = [fn(kind, d) for (_, fn), d in zip(variants, sides)]
        t_b, s_b = timed([lambda o=o, lv=lv, do=do: torch.autograd.grad(o, lv, do, retain_graph=True)
                          for o, lv, do in zip(outs, leaves, douts)])
        del outs
        for i, (tag, fn) in enumerate(variants):
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            o = fn(kind, sides[i])
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
        if kind == "down":      # dx = sub2x(dout: Cout -> Cin) on the coarse grid, dweight = corr(dout, x)
            row.update(kernel_tflops(HW // 2, cout, cin, g))
        elif kind == "up":      # forward = sub2x(x: Cin -> Cout) on the source grid, dweight = corr(x, dout)
            row.update(kernel_tflops(HW, cin, cout, g))
        print(json.dumps(row), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
