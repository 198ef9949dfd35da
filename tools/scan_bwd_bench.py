"""Selective-scan forward / backward times (founddiff_amd.selective_scan_train) at the SURVEY section 2a shapes of the
reference's training batch (train.py: train_batch_size = 2 at 512 x 512).  One JSON line per shape: fwd and bwd
milliseconds (median of --reps timed calls after --warmup) and the backward's effective bandwidth on its minimal traffic:
reads of u, delta, dout, B and C, writes of du, ddelta, dB and dC (the recompute pre-pass's second read of u, delta,
dout, B and C is not counted).

    python tools/scan_bwd_bench.py [--reps 20] [--warmup 3]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (level, KD, N, L) at K = 4 groups
SHAPES = [("down0", 512, 4, 65536), ("down1", 512, 8, 16384), ("down2", 1024, 16, 4096), ("down3", 2048, 32, 1024),
          ("mid", 4096, 32, 1024), ("ups0", 2048, 16, 4096), ("ups1", 1024, 8, 16384)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    from founddiff_amd import selective_scan_train as m
    dev = torch.device("cuda:0")
    b, K = a.batch, 4
    for name, KD, N, L in SHAPES:
        g = torch.Generator(device=dev).manual_seed(0)
        u = torch.randn(b, KD, L, device=dev, generator=g) * 0.5
        delta = torch.randn(b, KD, L, device=dev, generator=g) * 0.5 - 2
        A = -torch.rand(KD, N, device=dev, generator=g) - 0.5
        Bm = torch.randn(b, K, N, L, device=dev, generator=g)
        Cm = torch.randn(b, K, N, L, device=dev, generator=g)
        D, bias = torch.ones(KD, device=dev), torch.zeros(KD, device=dev)
        dout = torch.randn(b, KD, L, device=dev, generator=g)
        out, x = m.fwd(u, delta, A, Bm, Cm, D, bias, True, 1)

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

        t_f = timed(lambda: m.fwd(u, delta, A, Bm, Cm, D, bias, True, 1))
        t_b = timed(lambda: m.bwd(u, delta, A, Bm, Cm, D, bias, dout, x, True, 1))
        nbytes = 4 * (5 * b * KD * L + 4 * b * K * N * L)
        print(json.dumps(dict(shape=name, batch=b, KD=KD, K=K, N=N, L=L, fwd_ms=round(t_f, 4), bwd_ms=round(t_b, 4),
                              bwd_over_fwd=round(t_b / t_f, 2), bwd_min_bytes=nbytes,
                              bwd_eff_GBps=round(nbytes / t_b / 1e6, 1))), flush=True)
        del u, delta, Bm, Cm, dout, out, x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
