"""Ensembles without a GPU: the replica seeds (known answers, distinctness, range), the cut of the B * K rows into passes, and a gloo
world-2 run of sample_volume(n_samples=2) against world 1 with a stand-in that has the product's sample_ensemble interface."""
import os
import socket
from collections import namedtuple

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp


def test_ensemble_seeds_known_answers():
    from founddiff_amd.ensemble import ensemble_seeds
    assert ensemble_seeds([0], 3).tolist() == [[0, 811714673852932524, 1087295649107911329]]
    assert ensemble_seeds([7], 3).tolist() == [[7, 1737879033728604363, 1118851801103495394]]


def test_ensemble_seeds_shape_dtype_and_replica_zero():
    from founddiff_amd.ensemble import ensemble_seeds
    s = [5, 0, 2 ** 62 - 1, 123456789012345]
    for arg in (s, np.array(s, dtype=np.int64), torch.tensor(s, dtype=torch.int64)):
        out = ensemble_seeds(arg, 4)
        assert isinstance(out, np.ndarray) and out.dtype == np.int64 and out.shape == (4, 4)
        assert out[:, 0].tolist() == s                                     # replica 0 is the slice's own seed
    assert ensemble_seeds(s, 1).tolist() == [[v] for v in s]
    assert ensemble_seeds([], 3).shape == (0, 3)
    assert np.array_equal(ensemble_seeds(s, 4)[:, :2], ensemble_seeds(s, 2))     # replica k does not depend on K


def test_ensemble_seeds_distinct_and_in_range():
    from founddiff_amd.ensemble import ensemble_seeds
    seeds = list(range(4096)) + list(range(2 ** 62 - 64, 2 ** 62))
    out = ensemble_seeds(seeds, 16)
    assert out.size == 66560 and len(set(out.reshape(-1).tolist())) == 66560
    assert int(out.min()) >= 0 and int(out.max()) < 2 ** 62


def test_ensemble_seeds_raises():
    from founddiff_amd.ensemble import ensemble_seeds
    for bad_k in (0, -1):
        with pytest.raises(RuntimeError):
            ensemble_seeds([1], bad_k)
    for bad_seed in (-1, 2 ** 62, 2 ** 63 - 1):
        with pytest.raises(RuntimeError):
            ensemble_seeds([3, bad_seed], 2)


@pytest.mark.parametrize("B,K,rows_max", [(1, 1, 4), (3, 3, 4), (2, 4, 8), (1, 9, 4)])
def test_ensemble_passes(B, K, rows_max):
    from founddiff_amd.ensemble import ensemble_passes
    passes = ensemble_passes(B, K, rows_max)
    assert all(0 < hi - lo <= rows_max for lo, hi in passes)
    assert [r for lo, hi in passes for r in range(lo, hi)] == list(range(B * K))      # every row once, in order
    assert len(passes) == -(-B * K // rows_max)


def test_ensemble_passes_raises():
    from founddiff_amd.ensemble import ensemble_passes
    for args in ((1, 0, 4), (1, 2, 0)):
        with pytest.raises(RuntimeError):
            ensemble_passes(*args)


_Ens = namedtuple("_Ens", ["mean", "std", "spread", "samples"])


class _FakeEnsemble(torch.nn.Module):
    """sample_ensemble([x], K, slice_seeds) with a per-replica deterministic image: a function of the slice and of the replica's seed
    (ensemble_seeds; oracle/keyed_noise.py restates the keyed stream), as the product's is."""

    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))

    def sample_ensemble(self, x_input, n_samples, slice_seeds=None, return_samples=False):
        from founddiff_amd.ensemble import ensemble_seeds
        from oracle import keyed_noise
        x = x_input[0]
        rs = ensemble_seeds(slice_seeds, n_samples)
        assert rs.shape == (x.shape[0], n_samples)
        imgs = torch.stack([torch.stack([
            torch.tanh(x[b] * 3 - 0.25 * torch.from_numpy(keyed_noise.keyed_normal(int(rs[b, k]), 0x7FFFFFFF, x[b].numel())).view_as(x[b]))
            for k in range(n_samples)]) for b in range(x.shape[0])])
        std = imgs.std(1)
        return _Ens(imgs.mean(1), std, std.flatten(1).pow(2).mean(1).sqrt(), imgs if return_samples else None)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, n, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from founddiff_amd import parallel
    torch.manual_seed(0)
    vol = torch.rand(n, 1, 8, 8)
    mean, std = parallel.sample_volume(_FakeEnsemble(), vol, world=world, rank=rank, noise_seed=100, batch=2, n_samples=2)
    q.put((rank, mean, std))
    dist.barrier()
    dist.destroy_process_group()


def test_sample_volume_ensemble_sharded_equals_single():
    """Replicas are keyed by noise_seed + the GLOBAL slice index: (mean, std) of a world-2 run equal the world-1 run bitwise, and
    both volumes are gathered on every rank (5 slices: a ragged split)."""
    from founddiff_amd import parallel
    n = 5
    torch.manual_seed(0)
    vol = torch.rand(n, 1, 8, 8)
    ref_mean, ref_std = parallel.sample_volume(_FakeEnsemble(), vol, world=1, rank=0, noise_seed=100, batch=4, n_samples=2)
    assert ref_mean.shape == vol.shape and ref_std.shape == vol.shape and float(ref_std.min()) > 0
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, n, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert sorted(r for r, _, _ in res) == [0, 1]
    for _, mean, std in res:
        assert torch.equal(mean, ref_mean) and torch.equal(std, ref_std)
