"""The two outer convolutions of a training step through founddiff_amd.outer_conv_train (init_conv_fn, final_conv_fn) against what
unet_train.unet_trunk_forward does with init_fn = final_fn = None: nn.Conv2d on channels-last memory (and, for init_conv, the
permute to (B, H, W, C)), fp32, at the training shape (batch 2 from a 512 x 512 slice, dim 64).  Both sides run in the same process
on the same values.  One JSON line, also written to profiles/outer_conv_train_bench.json: per convolution the forward and backward
milliseconds of each side (median of --reps timed calls after --warmup, the two sides alternated call by call; the backward timed
from a graph built once and kept, retain_graph), torch.cuda.max_memory_allocated over one forward + backward above what the inputs
hold, and the two backward calls alone (fd_init_conv7_wgrad_f32, fd_final_conv1_bwd_f32) in GB/s against the bytes they must
move: dout once for the first (x and the gradient are 4 MB and 25 KB), x and dout read and dx written for the second.  Those are
times of a call's whole launch group (the kernel and its two launch_sum launches) between two device events, every repetition on
the same operands; they are not kernel times from a trace.  Before anything is timed the two sides' outputs and gradients are
compared at the timed size (rel_err = max |a - b| / max |b| against torch's fp32, reported as *_err; the run fails above the
project's gates of 1e-5 / 1e-4 / 1e-3 for outputs / activation gradients / parameter gradients).

    python tools/outer_conv_train_bench.py [--batch 2] [--size 512] [--dim 64] [--reps 20] [--warmup 3]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "outer_conv_train_bench.json"))
    a = ap.parse_args()
    from founddiff_amd import _lib as L
    from founddiff_amd.outer_conv_train import final_conv_fn, init_conv_fn
    dev = torch.device("cuda:0")
    B, S, C = a.batch, a.size, a.dim
    g = torch.Generator(device=dev).manual_seed(0)
    rn = lambda *s: torch.randn(*s, device=dev, generator=g)

    def timed(fns):
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

    def compare(tag, ours, theirs, leaves, douts, row, names):
        """ours / theirs: callables -> output; leaves: the tensors each differentiates; douts: the gradient of each output;
        names: (name, gate) of the output and of every leaf"""
        fns = (ours, theirs)
        got = [[o] + list(torch.autograd.grad(o, lv, do)) for o, lv, do in zip([fn() for fn in fns], leaves, douts)]
        for (name, gate), a_, b_ in zip(names, *got):
            a_, b_ = a_.detach().double(), b_.detach().double()
            err = float((a_ - b_).abs().max() / b_.abs().max())
            row[f"{tag}_{name}_err"] = float(f"{err:.2e}")
            if not err < gate:
                raise SystemExit(f"{tag}: {name} differs from torch's by {err:.2e} at the timed size (gate {gate:.0e})")
        del got
        with torch.no_grad():
            t_f, s_f = timed(list(fns))
        outs = [fn() for fn in fns]
        t_b, s_b = timed([lambda o=o, lv=lv, do=do: torch.autograd.grad(o, lv, do, retain_graph=True)
                          for o, lv, do in zip(outs, leaves, douts)])
        del outs
        for i, side in enumerate(("hip", "torch")):
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            o = fns[i]()
            torch.autograd.grad(o, leaves[i], douts[i])
            del o
            torch.cuda.synchronize()
            row.update({f"{tag}_{side}_fwd_ms": round(t_f[i], 3), f"{tag}_{side}_bwd_ms": round(t_b[i], 3),
                        f"{tag}_{side}_fwd_bwd_spread_ms": [round(s_f[i][0] + s_b[i][0], 3), round(s_f[i][1] + s_b[i][1], 3)],
                        f"{tag}_{side}_peak_MB": round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)})
        row[f"{tag}_speedup_fwd_bwd"] = round((row[f"{tag}_torch_fwd_ms"] + row[f"{tag}_torch_bwd_ms"]) /
                                              (row[f"{tag}_hip_fwd_ms"] + row[f"{tag}_hip_bwd_ms"]), 2)

    row = dict(tool="outer_conv_train_bench", batch=B, H=S, W=S, dim=C, reps=a.reps, device=torch.cuda.get_device_name(0))
    # ---- init_conv: x is data, the weight and the bias are differentiated
    x = rn(B, 2, S, S)
    conv = torch.nn.Conv2d(2, C, 7, padding=3).to(dev)
    w1, b1 = conv.weight.detach().clone().requires_grad_(), conv.bias.detach().clone().requires_grad_()
    dout = rn(B, S, S, C)
    compare("init", lambda: init_conv_fn(x, w1, b1),
            lambda: conv(x.contiguous(memory_format=torch.channels_last)).permute(0, 2, 3, 1).contiguous(),
            [[w1, b1], [conv.weight, conv.bias]], [dout, dout], row, (("out", 1e-5), ("dweight", 1e-3), ("dbias", 1e-3)))
    st = torch.cuda.current_stream().cuda_stream
    gbuf = torch.empty(99, C, device=dev)
    ws = torch.empty(max(4, int(L.lib().fd_init_conv7_wgrad_ws_floats(B, 2, S, S, C))), device=dev)
    (ms,), ((lo, hi),) = timed([lambda: L.call("fd_init_conv7_wgrad_f32", x.data_ptr(), dout.data_ptr(), gbuf.data_ptr(), ws.data_ptr(),
                                               B, 2, S, S, C, st)])
    nbytes = 4 * (dout.numel() + x.numel() + gbuf.numel())
    row.update(init_wgrad_ms=round(ms, 3), init_wgrad_spread_ms=[round(lo, 3), round(hi, 3)], init_wgrad_MB=round(nbytes / 2 ** 20, 1),
               init_wgrad_GBs=round(nbytes / (ms * 1e-3) / 1e9, 1),
               init_wgrad_TFLOPs=round(2.0 * dout.numel() * 98 / (ms * 1e-3) / 1e12, 2))
    del x, dout, gbuf, ws, conv
    # ---- final_conv: everything is differentiated
    xf = rn(B, S, S, C)
    conv = torch.nn.Conv2d(C, 1, 1).to(dev)
    w2, b2 = conv.weight.detach().clone().requires_grad_(), conv.bias.detach().clone().requires_grad_()
    xa, xb = xf.clone().requires_grad_(), xf.clone().requires_grad_()
    dout = rn(B, 1, S, S)
    compare("final", lambda: final_conv_fn(xa, w2, b2), lambda: conv(xb.permute(0, 3, 1, 2)),
            [[xa, w2, b2], [xb, conv.weight, conv.bias]], [dout, dout], row,
            (("out", 1e-5), ("dx", 1e-4), ("dweight", 1e-3), ("dbias", 1e-3)))
    dx, dwb = torch.empty_like(xf), torch.empty(C + 4, device=dev)
    ws = torch.empty(max(4, int(L.lib().fd_final_conv1_bwd_ws_floats(B * S * S, C))), device=dev)
    wv = w2.detach().view(C).contiguous()
    (ms,), ((lo, hi),) = timed([lambda: L.call("fd_final_conv1_bwd_f32", xf.data_ptr(), C, 0, wv.data_ptr(), dout.data_ptr(), dx.data_ptr(),
                                               dwb.data_ptr(), ws.data_ptr(), B * S * S, C, st)])
    nbytes = 4 * (2 * xf.numel() + dout.numel())
    row.update(final_bwd_ms=round(ms, 3), final_bwd_spread_ms=[round(lo, 3), round(hi, 3)], final_bwd_MB=round(nbytes / 2 ** 20, 1),
               final_bwd_GBs=round(nbytes / (ms * 1e-3) / 1e9, 1))
    line = json.dumps(row)
    print(line, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
