"""Data-parallel training, the parts that need no GPU: the numbering of the micro-batches (diffusion_train.dp_micro), the ordered
sum as a numpy statement (diffusion_train.ordered_sum), parallel.all_gather_flat over gloo with two processes, the arguments of
Trainer(data_parallel=True), and the declarations of csrc/fd_grad_sum.hip."""
import os
import re
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("fd_grads_tail_floats", "fd_grads_pack_f32", "fd_grads_rank_sum_f32")


def _draws(seed, step, m, batch, n, accumulate, T=1000, H=64, W=48, crop=32):
    """everything Trainer.train draws for micro-batch m of `accumulate`"""
    from founddiff_amd import diffusion_train as dt
    idx = dt.train_batch_indices(seed, step, m, batch, n, accumulate)
    t, seeds = dt.train_t_and_seeds(seed, step, m, idx, T)
    codes = dt.train_augment(seed, step, m, idx, square=True)
    windows = dt.train_crop(seed, step, m, idx, H, W, crop)
    return idx, t.tolist(), seeds.tolist(), codes.tolist(), windows.tolist()


@pytest.mark.parametrize("W,A", [(1, 4), (2, 2), (4, 1), (3, 2)])
def test_partition(W, A):
    """over ranks and rounds the new numbering covers the single process's micro-batches at accumulate = A W once each, draw for
    draw, and a round's ranks hold consecutive numbers in rank order (what makes the rank-ordered sum the global order)"""
    from founddiff_amd import diffusion_train as dt
    seed, batch, n = 5, 3, 7
    for step in (0, 1, 9):
        single = [_draws(seed, step, m, batch, n, A * W) for m in range(A * W)]
        seen = {}
        for a in range(A):
            row = [dt.dp_micro(a, W, r) for r in range(W)]
            assert row == list(range(a * W, (a + 1) * W))
            for r, m in enumerate(row):
                assert m not in seen
                seen[m] = _draws(seed, step, m, batch, n, A * W)
        assert sorted(seen) == list(range(A * W))
        assert [seen[m] for m in range(A * W)] == single
        # the samples of the step are those of the single process: consecutive numbers of the epoch's permutation
        flat = [i for m in range(A * W) for i in seen[m][0]]
        assert flat == [i for m in range(A * W) for i in dt.train_batch_indices(seed, step, m, batch, n, A * W)]
    with pytest.raises(RuntimeError):
        dt.dp_micro(0, 2, 2)
    with pytest.raises(RuntimeError):
        dt.train_batch_indices(seed, 0, A * W, batch, n, A * W)          # a number past the step's count is refused


def _mixed(rng, shape):
    """magnitudes far enough apart that the order of addition decides the result"""
    rounds, W, n = shape
    mags = np.array([1.0, -1.0, 1e-3, 3e4, -7e2, 4e5, 60.0, -9e3], dtype=np.float32)
    v = (mags[rng.integers(0, len(mags), (rounds * W, n))] * rng.uniform(0.5, 1.5, (rounds * W, n))).astype(np.float32)
    big = (1e8 * rng.uniform(0.5, 1.5, n)).astype(np.float32)
    slots = rng.random((rounds * W, n)).argsort(0)                       # per element: where +big and its exact negative go
    np.put_along_axis(v, slots[0:1], big[None], 0)
    if rounds * W >= 2:
        np.put_along_axis(v, slots[1:2], -big[None], 0)
    return v.reshape(rounds, W, n)


@pytest.mark.parametrize("W,rounds", [(1, 1), (2, 3), (3, 1), (8, 3)])
def test_ordered_sum(W, rounds):
    from founddiff_amd import diffusion_train as dt
    rng = np.random.default_rng(W * 10 + rounds)
    G = _mixed(rng, (rounds, W, 257))
    got = dt.ordered_sum([G[a] for a in range(rounds)])
    acc = np.zeros(257, dtype=np.float32)
    for m in range(rounds * W):                                          # global micro-batch m = a W + r, sequentially in float32
        acc = np.float32(acc) + G[m // W, m % W]
        assert acc.dtype == np.float32
    assert got.dtype == np.float32 and np.array_equal(got, acc)
    if W >= 2 and W * rounds >= 3:                                       # (two terms give one sum either way: addition commutes)
        rev = dt.ordered_sum([G[a][::-1] for a in range(rounds)])
        assert (rev != got).mean() >= 0.25                               # on these inputs another order is another result
    with pytest.raises(RuntimeError):
        dt.ordered_sum([])
    with pytest.raises(RuntimeError):
        dt.ordered_sum([G[0], G[0][:, :5]])


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _gather_worker(rank, world, port, q):
    import datetime
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    from founddiff_amd import parallel
    flat = torch.arange(11, dtype=torch.float32) + 100 * rank
    out = parallel.all_gather_flat(flat, torch.full((world, 11), -1.0))
    ints = parallel.gather_int64(7 + rank, torch.device("cpu"))
    w = torch.full((3,), float(rank + 1))
    parallel.broadcast_tensors([w], 0)
    bad = None
    try:
        parallel.all_gather_flat(flat, torch.zeros(world, 12))
    except RuntimeError as e:
        bad = str(e)
    q.put((rank, out, ints, w, bad))
    dist.barrier()
    dist.destroy_process_group()


def test_all_gather_flat_gloo():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gather_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    want = torch.stack([torch.arange(11, dtype=torch.float32) + 100 * r for r in range(2)])
    assert sorted(r[0] for r in res) == [0, 1]
    for _, out, ints, w, bad in res:
        assert torch.equal(out, want)                                    # rows in rank order, on every rank
        assert ints == [7, 8]
        assert torch.equal(w, torch.ones(3))
        assert bad is not None and "all_gather_flat" in bad and "inconsistent" in bad


def test_bad_arguments():
    import torch.distributed as dist
    from founddiff_amd import diffusion_train as dt, parallel
    from founddiff_amd.DADiff import Trainer
    assert not dist.is_initialized()
    with pytest.raises(RuntimeError, match="data_parallel=True needs an initialised process group"):
        Trainer(None, None, data_parallel=True)
    with pytest.raises(RuntimeError, match="not initialised"):
        parallel.all_gather_flat(torch.zeros(4), torch.zeros(1, 4))
    with pytest.raises(RuntimeError, match="ClipAdamEMA"):
        dt.GradReducer(object())
    import inspect
    sig = inspect.signature(Trainer.__init__).parameters
    assert sig["data_parallel"].default is False and sig["process_group"].default is None
    assert inspect.signature(dt.train_step).parameters["reducer"].default is None


def test_declarations():
    from founddiff_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "founddiff_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name in L.SIGNATURES and re.search(r"\bint " + name + r"\(", hdr), name
    assert len(L.SIGNATURES["fd_grads_pack_f32"][1]) == 10 and len(L.SIGNATURES["fd_grads_rank_sum_f32"][1]) == 12
    src = open(os.path.join(ROOT, "founddiff_amd", "csrc", "fd_grad_sum.hip")).read()
    code = "\n".join(ln.split("//")[0] for ln in src.splitlines())
    assert "fmaf" not in code and "atomic" not in code                   # plain adds in a fixed order
    for path in (L.LIB_PATH, L.LIB_F16_PATH):                            # the same entry points in both builds, where built
        if os.path.exists(path):
            import ctypes
            lib = ctypes.CDLL(path)
            assert all(hasattr(lib, name) for name in NEW_SYMBOLS)
            assert lib.fd_grads_tail_floats() == 4
