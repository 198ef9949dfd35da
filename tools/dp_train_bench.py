"""Data-parallel training (Trainer(data_parallel=True), diffusion_train.GradReducer, csrc/fd_grad_sum.hip): what the ordered gradient
sum costs.  Everything is reported, nothing is gated.  One JSON line per row, and all rows as one JSON line in --out:

  a  wall milliseconds per step of Trainer.train on the project's own model (dim 64, batch 2, 512 x 512, A = 2, log_every off): the
     plain path, which is the parent commit's
  b  the same with data_parallel=True at W = 1 over nccl, in the same process, the two loops alternated block by block: the
     overhead of pack + all-gather + rank-sum per micro-batch where nothing is gained
  c  W = min(device_count, 8) ranks, one process per device under torch.distributed.run, A W held at 2 where W divides it
     (W = 2: A = 1, ms per step), otherwise A = 1 and ms per micro-batch.  With one device this leg is named and not measured.
  k  the two kernels alone over the model's tables: fd_grads_pack_f32 (read + write + zero = 3 N floats) and
     fd_grads_rank_sum_f32 at W = 1 and at W = 8 rows (made here, not received), in the middle of a step ((W + 2) N floats) and as
     a step's only round (first and last: (W + 1) N): ms, GB/s, and the bytes over 6.3 TB/s as a floor
  g  parallel.all_gather_flat alone on the reducer's buffers at the W of this process (1: a device copy, no link is crossed)

Milliseconds in k and g are medians of --reps timed calls after --warmup, the variants alternated call by call.

    python tools/dp_train_bench.py [--batch 2] [--size 512] [--steps 10] [--warm 3] [--blocks 2] [--reps 20] [--warmup 3]
                                   [--legs a,b,c,k,g] [--out profiles/dp_train_bench.json]
"""
import argparse
import datetime
import json
import os
import socket
import subprocess
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T = 1000
HBM_BPS = 6.3e12
TINY_CLIP = dict(layers=(2, 1, 1, 1), width=16, embed_dim=1024)
PREFIX = "model.unet0."


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def make_trainer(folder, dev, B, S, A, items, **kw):
    from founddiff_amd import arch, synth
    from founddiff_amd.DADiff import ResidualDiffusion, Trainer, UnetRes, load_weights
    from founddiff_amd.data import DeviceSliceStore, SyntheticCTDataset
    w = synth.synth_state_dict(arch.da_unet_spec(64, (1, 2, 4, 8), prefix=PREFIX, clip=TINY_CLIP), seed=0)
    net = UnetRes(dim=64, dim_mults=(1, 2, 4, 8), num_unet=1, condition=True, objective="pred_res", test_res_or_noise="res",
                  precision="fp32", clip_cfg=TINY_CLIP)
    dif = ResidualDiffusion(net, image_size=S, timesteps=T, sampling_timesteps=2, objective="pred_res", loss_type="l1",
                            condition=True, sum_scale=0.01, test_res_or_noise="res")
    load_weights(dif, w, "synthetic weights")
    ds = SyntheticCTDataset(items, S, seed=10)
    store = DeviceSliceStore.from_dataset(ds, dev)
    return Trainer(None, dif.to(dev), checkpoint_folder=folder, dataset=ds, train_dataset=store, device=dev, train_batch_size=B,
                   gradient_accumulate_every=A, save_and_sample_every=10 ** 9, num_samples=1, train_num_steps=0, seed=5, log_every=0,
                   **kw)


def run_block(tr, steps):
    """wall milliseconds per step of `steps` more steps"""
    torch.cuda.synchronize()
    tr.train_num_steps = tr.step + steps
    t0 = time.perf_counter()
    tr.train()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def worker(a):
    """leg c: one rank of W under torch.distributed.run"""
    import torch.distributed as dist
    rank, world, local = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"]), int(os.environ.get("LOCAL_RANK", "0"))
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", device_id=dev, timeout=datetime.timedelta(seconds=300))
    A = 2 // world if 2 % world == 0 else 1
    with tempfile.TemporaryDirectory() as folder:
        tr = make_trainer(folder, dev, a.batch, a.size, A, a.items, data_parallel=True)
        run_block(tr, a.warm)
        ms = sorted(run_block(tr, a.steps) for _ in range(a.blocks))
    if rank == 0:
        row = dict(leg="c_data_parallel", W=world, A=A, batch=a.batch, size=a.size, ms_per_step=round(ms[len(ms) // 2], 3),
                   ms_per_micro_batch=round(ms[len(ms) // 2] / A, 3), micro_batches_per_step=A * world,
                   unit="ms per step at A W = 2" if A * world == 2 else "A W is not 2: compare ms_per_micro_batch")
        print("DP_ROW " + json.dumps(row), flush=True)
    dist.barrier()
    dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--items", type=int, default=16)
    ap.add_argument("--legs", default="a,b,c,k,g")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dp_train_bench.json"))
    ap.add_argument("--worker", action="store_true")
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    import torch.distributed as dist
    from founddiff_amd import parallel
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    legs, rows = a.legs.split(","), []
    B, S = a.batch, a.size

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    def timed(fns):
        ts = [[] for _ in fns]
        for it in range(a.warmup + a.reps):
            for i, fn in enumerate(fns):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if it >= a.warmup:
                    ts[i].append(e0.elapsed_time(e1))
        return [(sorted(v)[len(v) // 2], min(v)) for v in ts]

    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{free_port()}", rank=0, world_size=1, device_id=dev,
                            timeout=datetime.timedelta(seconds=300))
    with tempfile.TemporaryDirectory() as fa, tempfile.TemporaryDirectory() as fb:
        plain = make_trainer(fa, dev, B, S, 2, a.items) if "a" in legs or "b" in legs else None
        dp = make_trainer(fb, dev, B, S, 2, a.items, data_parallel=True) if set(legs) & {"b", "k", "g"} else None
        if plain is not None:
            run_block(plain, a.warm)
            run_block(dp, a.warm) if "b" in legs else None
            ta, tb = [], []
            for _ in range(a.blocks):
                ta.append(run_block(plain, a.steps))
                if "b" in legs:
                    tb.append(run_block(dp, a.steps))
            med = lambda v: sorted(v)[len(v) // 2]
            emit(dict(leg="a_plain", batch=B, size=S, A=2, ms_per_step=round(med(ta), 3), blocks=[round(v, 3) for v in ta],
                      steps_per_block=a.steps))
            if "b" in legs:
                same = all(torch.equal(p, q) for p, q in zip(plain.model.parameters(), dp.model.parameters()))
                emit(dict(leg="b_data_parallel_W1", batch=B, size=S, A=2, backend=dist.get_backend(), ms_per_step=round(med(tb), 3),
                          blocks=[round(v, 3) for v in tb], steps_per_block=a.steps, over_plain=round(med(tb) / med(ta), 4),
                          overhead_ms_per_micro_batch=round((med(tb) - med(ta)) / 2, 3), parameters_bitwise_equal_to_a=bool(same)))
        if dp is not None and ("k" in legs or "g" in legs):
            if dp._reducer is None:
                dp._setup_training()
            red, opt = dp._reducer, dp.opt0
            N = red.N
            for p in opt.params:
                p.grad = torch.randn_like(p) * 1e-3
            if "k" in legs:
                from founddiff_amd import _lib as L
                from founddiff_amd._train import ptr, stream
                red.pack([], zero=True)                  # uploads the pointer table; the timed calls are the launch alone
                st = stream(dev)
                (ms, mn), = timed([lambda: L.call("fd_grads_pack_f32", ptr(opt._chunks), ptr(opt._table), ptr(red._offs), opt.nchunk,
                                                  ptr(red.flat), red.P, None, 0, 1, st)])
                nbytes = 3 * 4 * N
                emit(dict(leg="k_fd_grads_pack_f32", N=N, ms=round(ms, 4), min_ms=round(mn, 4), MB=round(nbytes / 1e6, 1),
                          GBps=round(nbytes / ms / 1e6, 0), floor_ms_at_6300_GBps=round(nbytes / HBM_BPS * 1e3, 4),
                          fraction_of_6300_GBps=round(nbytes / (ms * 1e-3) / HBM_BPS, 3),
                          note="back-to-back calls on the same buffers: part of the bytes stays in the 256 MB Infinity Cache, so a "
                               "fraction above 1 is a cache figure, not an HBM one"))
                for W in (1, 8):
                    red.world, red.recv = W, torch.randn(W, N, device=dev) * 1e-3
                    res = timed([lambda: red.rank_sum(False, False), lambda: red.rank_sum(True, True)])
                    for (ms, mn), tag, floats in zip(res, ("middle_round", "only_round"), ((W + 2) * N, (W + 1) * N)):
                        nbytes = 4 * floats
                        emit(dict(leg="k_fd_grads_rank_sum_f32_" + tag, W=W, N=N, rows="made in place, not received", ms=round(ms, 4),
                                  min_ms=round(mn, 4), MB=round(nbytes / 1e6, 1), GBps=round(nbytes / ms / 1e6, 0),
                                  floor_ms_at_6300_GBps=round(nbytes / HBM_BPS * 1e3, 4),
                                  fraction_of_6300_GBps=round(nbytes / (ms * 1e-3) / HBM_BPS, 3)))
                red.world, red.recv = 1, torch.zeros(1, N, device=dev)
            if "g" in legs:
                (ms, mn), = timed([lambda: parallel.all_gather_flat(red.flat, red.recv, red.group)])
                emit(dict(leg="g_all_gather_flat", W=1, backend=dist.get_backend(), N=N, ms=round(ms, 4), min_ms=round(mn, 4),
                          MB_received=round(4 * N / 1e6, 1), note="W = 1: a copy on the device, no link is crossed"))
        del plain, dp
    dist.destroy_process_group()
    torch.cuda.empty_cache()
    if "c" in legs:
        W = min(torch.cuda.device_count(), 8)
        if W < 2:
            emit(dict(leg="c_data_parallel", W=W, measured=False,
                      note="one device: W >= 2 over RCCL and the scaling curve are NOT measured; from the link figures of SURVEY.md a "
                           "round at W = 8 receives 7 x 102 MB per rank, an ESTIMATE of a few ms against about 89 ms of compute per "
                           "micro-batch of two 512 x 512 slices"))
        else:
            cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={W}", "--master-addr", "127.0.0.1",
                   "--master-port", str(free_port()), os.path.abspath(__file__), "--worker", "--batch", str(B), "--size", str(S),
                   "--steps", str(a.steps), "--warm", str(a.warm), "--blocks", str(a.blocks), "--items", str(a.items)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=1200)
            got = [json.loads(ln[len("DP_ROW "):]) for ln in r.stdout.splitlines() if ln.startswith("DP_ROW ")]
            if r.returncode != 0 or not got:
                emit(dict(leg="c_data_parallel", W=W, measured=False, note="the worker run failed", stderr=r.stderr[-1500:]))
            else:
                emit(dict(got[0], measured=True))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(dict(tool="tools/dp_train_bench.py", batch=B, size=S, steps=a.steps, warm=a.warm, blocks=a.blocks,
                                    reps=a.reps, warmup=a.warmup, devices=torch.cuda.device_count(), rows=rows)) + "\n")


if __name__ == "__main__":
    main()
