"""Multi-GPU sampling: slices are independent units (each slice's reverse process depends only on
its own x_input / x_T / noise, src/DADiff.py:1276-1365; GroupNorm / LayerNorm are per-sample and
the RN50 BatchNorm runs in eval mode), so a volume shards over ranks by slice index with NO
collective on the data path.  The only exchange is one all-gather (RCCL over xGMI on GPUs,
gloo in the CPU tests) that reassembles the output volume.

Data-parallel training (Trainer(data_parallel=True)) exchanges more: all_gather_flat gathers every rank's flat gradient buffer
once per micro-batch, for diffusion_train.GradReducer to add the rows in rank order; broadcast_tensors and gather_int64 carry
rank 0's model at set-up and the replicas' fingerprints.
"""
import torch

from .tiling import tiled_ensemble_opt_in


def shard_range(n, world, rank):
    """Contiguous block split of range(n): rank r gets [lo, hi); ragged tails go to the last ranks."""
    per = (n + world - 1) // world
    lo = min(rank * per, n)
    return lo, min(lo + per, n)


def gather_volume(local, world, n_total=None):
    """All-gather equal-or-ragged per-rank blocks (B_local,1,H,W) into the full volume on every
    rank.  Ragged tails are padded to the largest block and masked on unpack."""
    if world == 1:
        return local
    import torch.distributed as dist
    per = torch.tensor([local.shape[0]], device=local.device, dtype=torch.int64)
    sizes = [torch.zeros_like(per) for _ in range(world)]
    dist.all_gather(sizes, per)
    sizes = [int(s.item()) for s in sizes]
    mx = max(sizes)
    pad = local
    if local.shape[0] < mx:
        pad = torch.cat([local, local.new_zeros((mx - local.shape[0],) + tuple(local.shape[1:]))], 0)
    out = torch.empty((world * mx,) + tuple(local.shape[1:]), device=local.device, dtype=local.dtype)
    dist.all_gather_into_tensor(out, pad.contiguous())
    if all(s == mx for s in sizes):
        vol = out
    else:
        vol = torch.cat([out[r * mx:r * mx + sizes[r]] for r in range(world)], 0)
    if n_total is not None:
        assert vol.shape[0] == n_total
    return vol


def sample_volume(diffusion, ldct, world=1, rank=0, noise_seed=0, batch=8, sampler_kwargs=None, n_samples=1, tile=None,
                  overlap=0, tile_fuse="final", tiled_ensemble=False, *, quantiles=None, orientations=None):
    """Denoise a whole volume ldct (N,1,H,W in [0,1], same tensor on every rank) with `diffusion`
    (a founddiff_amd.DADiff.ResidualDiffusion living on this rank's device).  x_T noise is keyed
    by the GLOBAL slice index, and so is the ancestral sampler's per-step noise (`slice_seeds`:
    fd_sched.hip's counter-based stream), so the result is invariant to `world` for both samplers.
    Returns the (N,1,H,W) volume on every rank.
    `n_samples` > 1: every slice is an ensemble of that many realisations (sample_ensemble) whose replica seeds derive from
    `noise_seed` + the GLOBAL slice index; returns (mean, std), two (N,1,H,W) volumes, on every rank.  `sampler_kwargs` are
    sample()'s and do not reach it.
    `tile` (an int or (th, tw); None: whole slices): every slice is sampled as overlapping tiles (sample_tiled with `overlap` and
    fuse=`tile_fuse`) under the slice seed `noise_seed` + its GLOBAL index; every row is keyed, so the volume is the same on any
    `world` and for any `batch`.  Together with n_samples > 1 it is opt-in: `tiled_ensemble=True` samples every slice as a tiled
    ensemble (sample_ensemble(tile=...)) under the same seeds and returns (mean, std) as above, the same on any `world` and for
    any `batch`; without the switch the combination raises (the raising default is pinned by tests).
    `quantiles` (keyword-only, with n_samples > 1; it raises otherwise): a sequence of Q levels in [0, 1]; returns (mean, std,
    quantiles), the third the (N,Q,1,H,W) volume of sample_ensemble(quantiles=...)'s maps, gathered like the first two.
    `orientations` (keyword-only; None: all of the above): "d4", "flips" or a sequence of flip / rot90 codes; every slice is an
    orientation ensemble (sample_ensemble(orientations=...)) of n_samples >= 1 replicas under the same seeds; returns (mean, std)
    as an ensemble does, at n_samples=1 too, the same on any `world` and for any `batch`.  Together with a tile it raises."""
    if orientations is not None and tile is not None:
        raise RuntimeError("sample_volume: orientation ensembles of tiled samples are not built")
    if quantiles is not None and int(n_samples) <= 1:
        raise RuntimeError(f"sample_volume: quantiles need an ensemble, n_samples > 1 (got {n_samples})")
    n = ldct.shape[0]
    lo, hi = shard_range(n, world, rank)
    dev = next(diffusion.parameters()).device
    tiled_ensemble_opt_in("sample_volume", tile, n_samples, tiled_ensemble)
    if tile is not None and int(n_samples) <= 1:
        outs = [diffusion.sample_tiled([ldct[s:min(s + batch, hi)].to(dev)], tile, overlap,
                                       slice_seeds=torch.arange(s, min(s + batch, hi), dtype=torch.int64) + int(noise_seed),
                                       fuse=tile_fuse)[-1]
                for s in range(lo, hi, batch)]
        local = torch.cat(outs, 0) if outs else ldct.new_zeros((0,) + tuple(ldct.shape[1:])).to(dev)
        return gather_volume(local, world, n)
    if int(n_samples) > 1 or orientations is not None:
        tkw = {} if tile is None else dict(tile=tile, overlap=overlap, tile_fuse=tile_fuse)
        if orientations is not None:
            tkw["orientations"] = orientations
        if quantiles is not None:
            tkw["quantiles"] = quantiles = tuple(float(q) for q in quantiles)
        means, stds, quants = [], [], []
        for s in range(lo, hi, batch):
            e = min(s + batch, hi)
            ens = diffusion.sample_ensemble([ldct[s:e].to(dev)], int(n_samples),
                                            slice_seeds=torch.arange(s, e, dtype=torch.int64) + int(noise_seed), **tkw)
            means.append(ens.mean)
            stds.append(ens.std)
            if quantiles is not None:
                quants.append(ens.quantiles)
        empty = ldct.new_zeros((0,) + tuple(ldct.shape[1:])).to(dev)
        vols = tuple(gather_volume(torch.cat(v, 0) if v else empty, world, n) for v in (means, stds))
        if quantiles is None:
            return vols
        empty_q = ldct.new_zeros((0, len(quantiles)) + tuple(ldct.shape[1:])).to(dev)
        return vols + (gather_volume(torch.cat(quants, 0) if quants else empty_q, world, n),)
    outs = []
    for s in range(lo, hi, batch):
        e = min(s + batch, hi)
        x = ldct[s:e].to(dev)
        nz = torch.stack([torch.randn(x.shape[1:], generator=torch.Generator().manual_seed(noise_seed + i))
                          for i in range(s, e)]).to(dev)
        seeds = torch.arange(s, e, dtype=torch.int64) + int(noise_seed)
        outs.append(diffusion.sample([x], batch_size=e - s, noise=nz, slice_seeds=seeds, **(sampler_kwargs or {}))[-1])
    local = torch.cat(outs, 0) if outs else ldct.new_zeros((0,) + tuple(ldct.shape[1:])).to(dev)
    return gather_volume(local, world, n)


# ---- data-parallel training: the exchanges of diffusion_train.GradReducer and of Trainer(data_parallel=True) ----------------------
_STAGE = {}      # (dtype, numel, world) -> (pinned send buffer, pinned receive buffer): the host staging of a non-nccl group


def _backend(group):
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        raise RuntimeError("parallel: torch.distributed is not initialised (call init_process_group first)")
    return dist.get_backend(group)


def all_gather_flat(flat, out, group=None):
    """out[r] = rank r's `flat`, on every rank: flat (N,) and out (W, N) dense, of one dtype and on one device, W the size of
    `group` (None: the default group).  On an nccl group this is dist.all_gather_into_tensor on the device buffers (RCCL).  On
    any other backend (gloo) device buffers are staged through pinned host memory -- down, all_gather, up, each waited for --
    and host buffers are gathered as they are.  Rows arrive in rank order whatever the backend: what a receiver does with them
    (diffusion_train's ordered sum) does not depend on how they travelled.  Returns out."""
    import torch.distributed as dist
    fn = "all_gather_flat"
    backend = _backend(group)
    W = dist.get_world_size(group)
    if not isinstance(flat, torch.Tensor) or not isinstance(out, torch.Tensor):
        raise RuntimeError(f"{fn}: flat and out must be tensors (got {type(flat).__name__}, {type(out).__name__})")
    if flat.dim() != 1 or tuple(out.shape) != (W, flat.numel()) or flat.dtype != out.dtype or flat.device != out.device or \
            not flat.is_contiguous() or not out.is_contiguous():
        raise RuntimeError(f"{fn}: inconsistent arguments flat{tuple(flat.shape)} {flat.dtype} on {flat.device}, out"
                           f"{tuple(out.shape)} {out.dtype} on {out.device} (flat (N,), out ({W}, N), dense, one dtype and device)")
    if backend == "nccl":
        if not flat.is_cuda:
            raise RuntimeError(f"{fn}: an nccl group gathers device buffers (flat lives on {flat.device})")
        dist.all_gather_into_tensor(out.view(-1), flat, group=group)
        return out
    if not flat.is_cuda:
        dist.all_gather([out[r] for r in range(W)], flat, group=group)
        return out
    key = (flat.dtype, flat.numel(), W)
    if key not in _STAGE:
        _STAGE[key] = (torch.empty(flat.numel(), dtype=flat.dtype).pin_memory(),
                       torch.empty(W, flat.numel(), dtype=flat.dtype).pin_memory())
    send, recv = _STAGE[key]
    send.copy_(flat)                                   # waits for the stream: the buffer is whole before it travels
    dist.all_gather([recv[r] for r in range(W)], send, group=group)
    out.copy_(recv)                                    # a blocking copy: recv is free again when this returns
    return out


def broadcast_tensors(tensors, src=0, group=None):
    """every tensor of `tensors` takes rank `src`'s values, in place: on the device over nccl, through the host otherwise"""
    import torch.distributed as dist
    backend = _backend(group)
    with torch.no_grad():
        for t in tensors:
            if backend == "nccl" or not t.is_cuda:
                dist.broadcast(t, src, group=group)
            else:
                h = t.detach().cpu()
                dist.broadcast(h, src, group=group)
                t.copy_(h)


def gather_int64(value, device, group=None):
    """[rank 0's value, rank 1's, ...] of one int64 per rank, on every rank (all_gather_flat on `device` for nccl, on the host
    otherwise)"""
    import torch.distributed as dist
    W = dist.get_world_size(group)
    dev = device if _backend(group) == "nccl" else torch.device("cpu")
    mine = torch.tensor([int(value)], dtype=torch.int64, device=dev)
    return all_gather_flat(mine, torch.empty(W, 1, dtype=torch.int64, device=dev), group).view(-1).cpu().tolist()
