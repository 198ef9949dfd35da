"""The fused adaLN / gated residual (founddiff_amd.adaln_train, csrc/fd_adaln_train.hip) against the torch composition it replaced
in mamba_block_train.mamba_block_forward -- F.layer_norm, 1 + scale, a multiply, an add, the gate multiply, the residual add -- at
the block shapes of the reference (train.py: batch 2 from a 512 x 512 slice; the level list of tools/tattn_train_bench.py, whose
seven entries cover the nine Mamba_blocks: ups.0 has the middle's shape and ups.3 that of downs.0).  One JSON line per shape:

  frame_*   the frame of one branch with the branch itself left out, x + gate * modulate(LayerNorm(x)): adaln_skip_fn +
            gate_residual_fn (two launches forward; two passes backward, the residual gradient joining dx inside the first)
            against the composition.  Forward and backward ms, peak MB of one forward + backward above what the inputs hold.
  kernel_*  each of the four C entries alone: ms per call, the bytes its algorithm has to move (every full-size tensor read or
            written once, plus the per-pixel statistics) and the GB/s that gives.  fd_adaln_bwd_f32 is timed with a dres.
  block_*   a whole MambaBlock, forward and backward ms and peak MB, against the same module with the composition as its frame.

The baseline (the composition) lives here, not in the package.  Milliseconds are medians of --reps timed calls after --warmup, the
two variants alternated call by call; the backward is timed from a graph built once and kept (retain_graph).

    python tools/adaln_train_bench.py [--batch 2] [--reps 10] [--warmup 2] [--shapes down0,mid] [--no-block]
"""
import argparse
import ctypes
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from tattn_train_bench import SHAPES  # noqa: E402  (level, image H = W, hidden size C)

D_STATE = {512: 4, 256: 8, 128: 16, 64: 32}        # the reference's d_state at each resolution
TIME_DIM = 256


def modulate(x, shift, scale):
    return x * (1 + scale[:, None, None, :]) + shift[:, None, None, :]


def frame_comp(p):
    C = p["x"].shape[-1]
    shift, scale, gate = p["mod"][:, :C], p["mod"][:, C:2 * C], p["mod"][:, 2 * C:3 * C]
    return p["x"] + gate[:, None, None, :] * modulate(F.layer_norm(p["x"], (C,), p["gamma"], p["beta"], 1e-5), shift, scale)


def frame_fused(p):
    from founddiff_amd.adaln_train import adaln_skip_fn, gate_residual_fn
    C = p["x"].shape[-1]
    shift, scale, gate = p["mod"][:, :C], p["mod"][:, C:2 * C], p["mod"][:, 2 * C:3 * C]
    m, skip = adaln_skip_fn(p["x"], p["gamma"], p["beta"], shift, scale, 1e-5)
    return gate_residual_fn(skip, m, gate)


def block_comp(self, x, c, t):
    """mamba_block_forward as it was before the fused frame: the LayerNorms, modulate, the gates and the adds with torch"""
    from founddiff_amd.ss2d_train import ss2d_forward
    from founddiff_amd.tattn_train import transposed_attention_nhwc
    x = x.permute(0, 2, 3, 1)
    shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp = self.adaLN_modulation(t).chunk(6, dim=1)
    x = x + gate_msa[:, None, None, :] * ss2d_forward(self.mamba, modulate(self.norm1(x), shift_msa, scale_msa), c)
    x = x + gate_mlp[:, None, None, :] * transposed_attention_nhwc(self.attn_blk, modulate(self.norm2(x), shift_mlp, scale_mlp))
    return x.permute(0, 3, 1, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default=",".join(s[0] for s in SHAPES))
    ap.add_argument("--no-block", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    b = a.batch
    from founddiff_amd import _lib as L
    from founddiff_amd.mamba_block_train import MambaBlock, mamba_block_forward

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
        return [sorted(t)[len(t) // 2] for t in ts]

    def peak(fn, leaves, dout):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        o = fn()
        torch.autograd.grad(o, leaves, dout)
        del o
        torch.cuda.synchronize()
        mb = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
        torch.cuda.empty_cache()
        return round(mb, 1)

    def compare(row, key, variants, leaves, dout):
        """fwd / bwd ms and peak MB of ("fused", fn), ("comp", fn) into row under key_*"""
        with torch.no_grad():
            t_f = timed([fn for _, fn in variants])
        outs = [fn() for _, fn in variants]
        t_b = timed([lambda o=o: torch.autograd.grad(o, leaves, dout, retain_graph=True) for o in outs])
        del outs
        for i, (tag, fn) in enumerate(variants):
            row.update({f"{key}_{tag}_fwd_ms": round(t_f[i], 3), f"{key}_{tag}_bwd_ms": round(t_b[i], 3),
                        f"{key}_{tag}_peak_MB": peak(fn, leaves, dout)})
        tot = lambda tag: row[f"{key}_{tag}_fwd_ms"] + row[f"{key}_{tag}_bwd_ms"]
        row[f"{key}_speedup_fwd_bwd"] = round(tot("comp") / tot("fused"), 2)
        row[f"{key}_memory_ratio"] = round(row[f"{key}_fused_peak_MB"] / row[f"{key}_comp_peak_MB"], 3)

    for name, HW, C in SHAPES:
        if name not in a.shapes.split(","):
            continue
        g = torch.Generator(device=dev).manual_seed(0)
        rn = lambda *s: torch.randn(*s, device=dev, generator=g)
        row = dict(shape=name, batch=b, H=HW, W=HW, C=C)
        hw = HW * HW
        # ---- the frame of one branch
        p = dict(x=rn(b, HW, HW, C), gamma=1 + 0.3 * rn(C), beta=0.3 * rn(C), mod=0.3 * rn(b, 6 * C))
        p = {k: v.requires_grad_() for k, v in p.items()}
        dout = rn(b, HW, HW, C)
        compare(row, "frame", (("fused", lambda: frame_fused(p)), ("comp", lambda: frame_comp(p))), list(p.values()), dout)
        # ---- the four entries alone
        with torch.no_grad():
            x, mod, gamma, beta = p["x"].detach(), p["mod"].detach(), p["gamma"].detach(), p["beta"].detach()
            y, dres = rn(b, HW, HW, C), rn(b, HW, HW, C)
            out, stats, dmod = torch.empty_like(x), torch.empty(b, HW, HW, 2, device=dev), torch.empty(b, 6 * C, device=dev)
            dg, db = torch.empty(C, device=dev), torch.empty(C, device=dev)
            ws = torch.empty(max(L.lib().fd_adaln_bwd_ws_floats(b, hw, C), 4), device=dev)
            st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            P = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + 4 * off)
            n4 = 4 * b * hw * C                                          # bytes of one full-size tensor
            sb = 8 * b * hw                                              # of the statistics
            entries = (
                ("adaln_fwd", 2 * n4 + sb, lambda: L.call("fd_adaln_fwd_f32", P(x), P(gamma), P(beta), 1e-5, P(mod), P(mod, C), 6 * C,
                                                          P(out), P(stats), b, hw, C, st)),
                ("adaln_bwd", 4 * n4 + sb, lambda: L.call("fd_adaln_bwd_f32", P(dout), P(x), P(stats), P(gamma), P(beta), P(mod, C),
                                                          6 * C, P(dres), P(out), P(dmod), P(dmod, C), 6 * C, P(dg), P(db), P(ws), b,
                                                          hw, C, st)),
                ("gate_res_fwd", 3 * n4, lambda: L.call("fd_gate_res_fwd_f32", P(x), P(y), P(mod, 2 * C), 6 * C, P(out), b, hw, C, st)),
                ("gate_res_bwd", 3 * n4, lambda: L.call("fd_gate_res_bwd_f32", P(dout), P(y), P(mod, 2 * C), 6 * C, P(out),
                                                        P(dmod, 2 * C), 6 * C, P(ws), b, hw, C, st)),
            )
            for (tag, nbytes, _), ms in zip(entries, timed([fn for _, _, fn in entries])):
                row.update({f"kernel_{tag}_ms": round(ms, 4), f"kernel_{tag}_MB": round(nbytes / 1e6, 1),
                            f"kernel_{tag}_GBps": round(nbytes / ms / 1e6, 0)})
            del x, mod, gamma, beta, y, dres, out, stats, ws
        del p, dout
        torch.cuda.empty_cache()
        # ---- a whole block
        if not a.no_block:
            torch.manual_seed(0)
            m = MambaBlock(C, D_STATE[HW], TIME_DIM)
            with torch.no_grad():
                for q in m.adaLN_modulation[-1].parameters():
                    q.copy_(0.1 * torch.randn_like(q))
            m = m.to(dev)
            xb, cb, tb = rn(b, HW, HW, C).permute(0, 3, 1, 2).requires_grad_(), rn(b, 1, 256), rn(b, TIME_DIM)
            dout = rn(b, HW, HW, C).permute(0, 3, 1, 2)
            leaves = [xb] + list(m.parameters())
            compare(row, "block", (("fused", lambda: mamba_block_forward(m, xb, cb, tb)), ("comp", lambda: block_comp(m, xb, cb, tb))),
                    leaves, dout)
            del m, xb, cb, tb, dout, leaves
            torch.cuda.empty_cache()
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
