"""Worker of tests/test_gpu_dp_train.py, launched by torch.distributed.run: Trainer(data_parallel=True) on the model of
tests/test_gpu_own_train.py (dim 64, mults (1, 2), 64 x 64, TINY_CLIP, SyntheticCTDataset(6, 64)).  The builders below are also what
the parent process makes its single-process runs with, so both sides differ in the data-parallel arguments alone.

    python _dp_train_worker.py <out_dir> w2     two ranks (nccl on two devices, or gloo with both ranks on cuda:0): the three
                                                configurations, 3 steps each at A = 1, then 2 steps and save(1) for the resume
    python _dp_train_worker.py <out_dir> w1     one rank over nccl: the host configuration at A = 2, 3 steps

Every rank writes <out_dir>/<name>_rank<r>.pt = its state, counters, logged losses and the fingerprints of the last replica check."""
import datetime
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
import torch  # noqa: E402

TINY_CLIP = dict(layers=(2, 1, 1, 1), width=16, embed_dim=1024)
DIM, MULTS, SIZE, T = 64, (1, 2), 64, 1000
CONFIGS = ("host", "store", "two")


def weights(two):
    from founddiff_amd import arch, synth
    w = dict(synth.synth_state_dict(arch.da_unet_spec(DIM, MULTS, prefix="model.unet0.", clip=TINY_CLIP), seed=0))
    if two:
        w.update(synth.synth_state_dict(arch.da_unet_spec(DIM, MULTS, prefix="model.unet1.", clip=TINY_CLIP), seed=1))
    return w


def diffusion(two, dev):
    from founddiff_amd.DADiff import ResidualDiffusion, UnetRes, load_weights
    objective, test = ("pred_res_noise", "res_noise") if two else ("pred_res", "res")
    net = UnetRes(dim=DIM, dim_mults=MULTS, num_unet=2 if two else 1, condition=True, objective=objective, test_res_or_noise=test,
                  precision="fp32", clip_cfg=TINY_CLIP)
    dif = ResidualDiffusion(net, image_size=SIZE, timesteps=T, sampling_timesteps=2, objective=objective, loss_type="l1",
                            condition=True, sum_scale=0.01, test_res_or_noise=test)
    load_weights(dif, weights(two), "synthetic weights")
    return dif.to(dev)


def trainer(folder, steps, config, dev="cuda", **kw):
    """config 'host': a host dataset; 'store': a DeviceSliceStore with augment=True, crop_size=32; 'two': two U-Nets under RAdam"""
    from founddiff_amd.DADiff import Trainer
    from founddiff_amd.data import DeviceSliceStore, SyntheticCTDataset
    ds = SyntheticCTDataset(6, SIZE, seed=10)
    args = dict(train_batch_size=2, gradient_accumulate_every=2, save_and_sample_every=100, train_lr=1e-3, ema_update_every=1,
                num_samples=4, train_num_steps=steps, seed=5, log_every=1)
    train = ds
    if config == "store":
        train = DeviceSliceStore.from_dataset(ds, dev)
        args.update(augment=True, crop_size=32)
    if config == "two":
        args.update(optimizer="radam")
    args.update(kw)
    return Trainer(None, diffusion(config == "two", dev), checkpoint_folder=str(folder), dataset=ds, train_dataset=train, device=dev,
                   **args)


def state(tr):
    """every parameter, EMA tensor and optimiser tensor as CPU tensors; the counters; the logged losses"""
    out = {"model." + k: v.detach().cpu().clone() for k, v in tr.model.state_dict().items()}
    out.update({"ema." + k: v.detach().cpu().clone() for k, v in tr.ema.ema_model.state_dict().items()})
    out.update({f"exp_avg.{i}": v.cpu().clone() for i, v in enumerate(tr.opt0.exp_avg)})
    out.update({f"exp_avg_sq.{i}": v.cpu().clone() for i, v in enumerate(tr.opt0.exp_avg_sq)})
    return {"tensors": out, "counters": (tr.step, tr.opt0.ema_step, tr.opt0.ema_copied, tr.opt0.steps()),
            "losses": list(tr.loss_log), "batch_log": list(tr.batch_log), "fingerprints": tr.fingerprints}


def main():
    import torch.distributed as dist
    out_dir, mode = sys.argv[1], sys.argv[2]
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    local = int(os.environ.get("LOCAL_RANK", "0"))
    nccl = mode == "w1" or torch.cuda.device_count() >= 2
    dev = torch.device("cuda", local if nccl else 0)
    torch.cuda.set_device(dev)
    limit = datetime.timedelta(seconds=120)              # a lost peer ends in an error, not a hang
    if nccl:
        dist.init_process_group("nccl", device_id=dev, timeout=limit)
    else:
        dist.init_process_group("gloo", timeout=limit)
    info = {"backend": dist.get_backend(), "world": world, "device": dev.index}
    if mode == "w1":
        tr = trainer(os.path.join(out_dir, "w1"), 3, "host", dev, data_parallel=True)
        tr.train()
        torch.save(dict(state(tr), **info), os.path.join(out_dir, f"w1_rank{rank}.pt"))
    else:
        for config in CONFIGS:
            tr = trainer(os.path.join(out_dir, config), 3, config, dev, gradient_accumulate_every=1, data_parallel=True)
            assert tr.accelerator.is_main_process == (rank == 0)
            tr.train()
            torch.save(dict(state(tr), **info), os.path.join(out_dir, f"{config}_rank{rank}.pt"))
            del tr
        tr = trainer(os.path.join(out_dir, "resume"), 2, "host", dev, gradient_accumulate_every=1, data_parallel=True)
        tr.train()
        tr.save(1)                                       # every rank joins: rank 0 writes, a barrier, the replica check
        torch.save(dict(state(tr), **info), os.path.join(out_dir, f"resume_rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
