"""founddiff_amd.data.DeviceSliceStore and diffusion_train.StoreBatch (csrc/fd_train_data.hip) on the GPU: the gather against numpy's
flip / rot90, the fused q_sample against the gather followed by the existing q_sample, NDCT de-duplication, and Trainer.train from
a store, with and without augmentation, against the host path.  Every comparison is bitwise: copies, or identical arithmetic.

Shapes: 64 (one tile), 72 (partial tiles, 16-byte path), 70 (W % 4 != 0: the per-pixel path, odd k included), 130 (3 x 3 tiles,
ragged, per pixel), and 48 x 80 (not square: the 8 codes with an even k)."""
import functools

import numpy as np
import pytest
import torch

from test_train_data_cpu import numpy_augment

pytestmark = pytest.mark.gpu
SHAPES = [(64, 64), (72, 72), (70, 70), (130, 130), (48, 80)]
ND_INDEX = [0, 1, 1, 2, 0]            # items 1 and 2 (and 0 and 4) share one stored NDCT
T = 1000


def _codes(H, W):
    return [c for c in range(16) if H == W or not c & 4]


@functools.lru_cache(maxsize=None)
def _store(H, W):
    """(store, nd, ld): random slices on the host and their store; unchanged by every test"""
    from founddiff_amd.data import DeviceSliceStore
    rng = np.random.default_rng(H * 1000 + W)
    nd, ld = rng.random((3, H, W), dtype=np.float32), rng.random((len(ND_INDEX), H, W), dtype=np.float32)
    return DeviceSliceStore(torch.from_numpy(nd).cuda(), torch.from_numpy(ld).cuda(), ND_INDEX), nd, ld


def _expect(nd, ld, indices, codes):
    xs = np.stack([numpy_augment(nd[ND_INDEX[i]][None], c) for i, c in zip(indices, codes)])
    xi = np.stack([numpy_augment(ld[i][None], c) for i, c in zip(indices, codes)])
    return xs, xi


@pytest.mark.parametrize("H,W", SHAPES)
def test_batch_against_numpy(H, W):
    store, nd, ld = _store(H, W)
    assert len(store) == 5 and store.n_nd == 3 and store.nbytes == 4 * 8 * H * W + 40
    assert store.nd_index_dev.is_cuda and store.nd_index_dev.tolist() == ND_INDEX and store.nd_index.tolist() == ND_INDEX
    codes = _codes(H, W)
    indices = [(3 * k + 1) % 5 for k in range(len(codes))]               # every item several times, items 1 and 2 among them
    xs, xi = store.batch(indices, codes)
    es, ei = _expect(nd, ld, indices, codes)
    assert xs.shape == xi.shape == (len(codes), 1, H, W) and xs.is_cuda
    bad = [c for k, c in enumerate(codes) if not (np.array_equal(xs[k].cpu().numpy(), es[k]) and
                                                  np.array_equal(xi[k].cpu().numpy(), ei[k]))]
    assert not bad, bad
    # three different codes in one call (both forms side by side on a square store), a repeated index, and no codes at all
    three = [9, 2, 6] if H == W else [9, 2, 3]
    xs, xi = store.batch([4, 4, 0], three)
    es, ei = _expect(nd, ld, [4, 4, 0], three)
    assert np.array_equal(xs.cpu().numpy(), es) and np.array_equal(xi.cpu().numpy(), ei)
    xs, xi = store.batch([1, 2])
    assert torch.equal(xs[0], xs[1]) and not torch.equal(xi[0], xi[1])   # one stored NDCT behind two items
    assert np.array_equal(xs.cpu().numpy()[:, 0], nd[[1, 1]]) and np.array_equal(xi.cpu().numpy()[:, 0], ld[[1, 2]])
    # the dataset surface: device views of the stored slices
    a, b = store[2]
    assert a.shape == b.shape == (1, H, W) and a.data_ptr() == store.nd[1].data_ptr() and b.data_ptr() == store.ld[2].data_ptr()
    with pytest.raises(IndexError):
        store[5]
    with pytest.raises(RuntimeError, match="outside"):
        store.batch([5])


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("H,W", SHAPES)
def test_fused_equals_composed(H, W, normalize):
    """q_sample(StoreBatch) against store.batch() followed by the existing q_sample: x_in, x_res, noise, times and x0, with keyed
    noise and with given noise"""
    from founddiff_amd import diffusion_train as dt
    from founddiff_amd.DADiff import residual_schedule
    store, _, _ = _store(H, W)
    sch = residual_schedule(T)
    codes = _codes(H, W)
    B = len(codes)
    indices = [(3 * k + 1) % 5 for k in range(B)]
    rng = np.random.default_rng(7)
    t = rng.integers(0, T, B, dtype=np.int64)
    seeds = rng.integers(0, 1 << 62, B, dtype=np.int64)
    noise = torch.randn(B, 1, H, W, generator=torch.Generator().manual_seed(3)).cuda()
    xs, xi = store.batch(indices, codes)
    sb = dt.StoreBatch(store, indices, codes)
    names = ("x_in", "x_res", "noise", "times", "x0")
    for kind, kw_dev, kw_host in (("keyed", dict(slice_seeds=torch.from_numpy(seeds).cuda(), step=11), dict(slice_seeds=seeds, step=11)),
                                  ("given", dict(noise=noise), dict(noise=noise))):
        want = dt.q_sample(xs, xi, torch.from_numpy(t).cuda(), sch, normalize=normalize, x0_out=True, **kw_dev)
        got = dt.q_sample(sb, None, t, sch, normalize=normalize, x0_out=True, **kw_host)
        assert len(got) == len(want) == 5
        bad = [n for n, g, w in zip(names, got, want) if g.shape != w.shape or not torch.equal(g, w)]
        assert not bad, (kind, bad)
        assert torch.equal(got[4], xs * 2 - 1 if normalize else xs)
        # t and the seeds as tensors on the device give the same, and so does the four-result form
        again = dt.q_sample(sb, None, torch.from_numpy(t).cuda(), sch, normalize=normalize, **kw_dev)
        assert len(again) == 4 and all(torch.equal(g, w) for g, w in zip(again, want))
    assert not torch.equal(got[0][:, 1], (xs * 2 - 1 if normalize else xs)[:, 0])        # the batch is not degenerate


def test_p_losses_and_train_step_take_a_store_batch():
    """p_losses_fn on a StoreBatch equals p_losses_fn on the gathered batch, for an objective with one target and for
    pred_x0_noise (the x0 output); train_step takes one StoreBatch, or a list of them"""
    from founddiff_amd import diffusion_train as dt
    from founddiff_amd.DADiff import residual_schedule
    store, _, _ = _store(72, 72)
    sch = residual_schedule(T)
    indices, codes, t, seeds = [0, 3, 3], [13, 2, 7], np.array([10, 500, 999]), np.array([5, 6, 7])
    w = torch.nn.Parameter(torch.full((1,), 0.5, device="cuda"))
    one = lambda x, times: [x[:, :1] * w]
    two = lambda x, times: [x[:, :1] * w, x[:, 1:] * w]
    xs, xi = store.batch(indices, codes)
    sb = dt.StoreBatch(store, indices, codes)
    for fn, objective in ((one, "pred_res"), (two, "pred_x0_noise")):
        for normalize in (True, False):
            want = dt.p_losses_fn(fn, [xs, xi], torch.from_numpy(t).cuda(), sch, objective, "l2", None, torch.from_numpy(seeds).cuda(),
                                  4, 1.0, normalize)
            got = dt.p_losses_fn(fn, sb, t, sch, objective, "l2", None, seeds, 4, 1.0, normalize)
            assert len(got) == len(want) and all(torch.equal(g, v) for g, v in zip(got, want)), (objective, normalize)
    opt = dt.ClipAdamEMA([w], lr=1e-2)
    a = dt.train_step(one, opt, sb, t, None, seeds, 4, sch)
    b = dt.train_step(one, opt, [sb, sb], [t, t], None, [seeds, seeds], 4, sch)
    assert len(a) == len(b) == 1 and bool(torch.isfinite(a[0])) and bool(torch.isfinite(b[0])) and float(w.detach()) != 0.5


def test_mixed_dose_store_shares_ndct(tmp_path):
    """two dose levels over three full-dose slices, written with save_slice: n_nd = 3 < n_ld = 6, and every item equals the host
    dataset's, bit for bit"""
    from founddiff_amd import data
    rng = np.random.default_rng(2)
    full, q = [], []
    for i in range(3):
        p = tmp_path / f"ab-full_1mm-{i:04d}.npy"
        data.save_slice(str(p), rng.random((20, 24), dtype=np.float32))
        full.append(str(p))
    for dose in ("0.25", "0.10"):
        for i in (2, 0, 1):
            p = tmp_path / f"ab-sim-{dose}-{i:04d}.npy"
            data.save_slice(str(p), rng.random((20, 24), dtype=np.float32))
            q.append(str(p))
    ds = data.MixedDoseTestDataset(q, {"ab": full})
    store = data.DeviceSliceStore.from_mixed_dose(ds, "cuda")
    assert len(store) == 6 and store.n_nd == 3 and store.n_nd < store.n_ld and (store.H, store.W) == (20, 24)
    assert store.nd_index.tolist() == [0, 1, 2, 0, 1, 2]
    for i in range(6):
        (a, b), (ha, hb) = store[i], ds[i]
        assert torch.equal(a.cpu(), ha) and torch.equal(b.cpu(), hb), i
        assert store.load_name(i) == ds.load_name(i)
    xs, xi = store.batch([3, 0], [3, 8])
    assert torch.equal(xs[0, 0].cpu(), ds[3][0][0].flip(0, 1)) and torch.equal(xi[1, 0].cpu(), ds[0][1][0].flip(0, 1))
    # from_dataset keeps one NDCT per item and the names
    plain = data.DeviceSliceStore.from_dataset(ds, "cuda")
    assert plain.n_nd == plain.n_ld == 6 and plain.load_name(4) == ds.load_name(4)
    assert all(torch.equal(plain[i][0], store[i][0]) and torch.equal(plain[i][1], store[i][1]) for i in range(6))


# ---- Trainer.train: Unet(64, (1, 2)) on 64 x 64 phantoms, batch 2, two micro-batches, as tests/test_gpu_own_train.py ---------------
def _dataset():
    from founddiff_amd.data import SyntheticCTDataset
    return SyntheticCTDataset(6, 64, seed=10)


def _trainer(folder, steps, from_store, augment):
    from founddiff_amd.DADiff import Trainer
    from founddiff_amd.data import DeviceSliceStore
    from test_gpu_own_train import _diffusion
    ds = _dataset()
    train = DeviceSliceStore.from_dataset(ds, "cuda") if from_store else ds
    return Trainer(None, _diffusion(), checkpoint_folder=str(folder), dataset=ds, train_dataset=train, device="cuda", train_batch_size=2,
                   gradient_accumulate_every=2, save_and_sample_every=100, train_lr=1e-3, ema_update_every=1, num_samples=4,
                   train_num_steps=steps, seed=5, log_every=2, augment=augment)


_RUNS = {}


def _run(tmp_path_factory, from_store, augment, tag=""):
    """the state after two steps (every parameter, EMA and Adam tensor, as CPU tensors), the counters and the batch log; each run
    is made once"""
    from test_gpu_own_train import _state
    key = (from_store, augment, tag)
    if key not in _RUNS:
        tr = _trainer(tmp_path_factory.mktemp("run"), 2, from_store, augment)
        tr.train()
        _RUNS[key] = _state(tr) + (list(tr.batch_log),)
    return _RUNS[key]


def _differ(a, b):
    return [k for k in a if not torch.equal(a[k], b[k])]


def test_trainer_store_equals_host(tmp_path_factory):
    host, ch, lh = _run(tmp_path_factory, False, False)
    store, cs, ls = _run(tmp_path_factory, True, False)
    assert ch == cs and lh == ls and len(lh) == 4 and sorted(host) == sorted(store)
    assert not _differ(host, store), _differ(host, store)[:5]


def test_trainer_augmented_repeats_and_differs(tmp_path_factory):
    a, ca, la = _run(tmp_path_factory, True, True)
    b, cb, lb = _run(tmp_path_factory, True, True, "again")
    assert ca == cb and la == lb and not _differ(a, b), _differ(a, b)[:5]
    plain, _, lp = _run(tmp_path_factory, True, False)
    assert lp == la                                                      # the same items ...
    assert _differ(a, plain)                                             # ... under other transforms: other weights


def test_trainer_augmented_host_and_store_agree(tmp_path_factory):
    a, ca, la = _run(tmp_path_factory, True, True)
    h, ch, lh = _run(tmp_path_factory, False, True)
    assert ca == ch and la == lh and not _differ(a, h), _differ(a, h)[:5]


def test_trainer_augmented_resumes(tmp_path_factory):
    a, ca, la = _run(tmp_path_factory, True, True)
    folder = tmp_path_factory.mktemp("resume")
    from test_gpu_own_train import _state
    first = _trainer(folder, 1, True, True)
    first.train()
    first.save(1)
    second = _trainer(folder, 2, True, True)
    second.load(1, for_training=True)
    assert second.step == 1
    second.train()
    b, cb = _state(second)
    assert cb == ca and first.batch_log + second.batch_log == la
    assert not _differ(a, b), _differ(a, b)[:5]


class _Stop(Exception):
    pass


def test_trainer_assembles_the_augmented_batch(tmp_path, monkeypatch):
    """the first micro-batch train() hands to the step, gathered, equals numpy's flip / rot90 of the logged items under
    train_augment's codes -- from a store and from a host dataset"""
    from founddiff_amd import diffusion_train as dt
    ds = _dataset()
    for from_store in (True, False):
        seen = []

        def stop(model, opt, batches, **kw):
            seen.append((batches, kw))
            raise _Stop                                                  # nothing is trained here
        monkeypatch.setattr(dt, "train_step", stop)
        tr = _trainer(tmp_path / str(from_store), 1, from_store, True)
        with pytest.raises(_Stop):
            tr.train()
        batches, kw = seen[0]
        assert len(batches) == 2 and all(isinstance(b, dt.StoreBatch) for b in batches) and kw["step"] == 0
        for m, sb in enumerate(batches):
            idx = tr.batch_log[m]
            codes = dt.train_augment(5, 0, m, idx)
            assert idx == dt.train_batch_indices(5, 0, m, 2, 6, 2) and sb.codes.tolist() == codes.tolist()
            assert sb.indices.tolist() == (idx if from_store else [0, 1])
            t, seeds = dt.train_t_and_seeds(5, 0, m, idx, T)
            assert np.array_equal(kw["t"][m], t) and np.array_equal(kw["slice_seeds"][m], seeds)
            xs, xi = sb.store.batch(sb.indices, sb.codes)
            for k, (i, c) in enumerate(zip(idx, codes)):
                nd, ld = ds[i]
                assert np.array_equal(xs[k].cpu().numpy(), numpy_augment(nd.numpy(), int(c))), (m, k)
                assert np.array_equal(xi[k].cpu().numpy(), numpy_augment(ld.numpy(), int(c))), (m, k)
        monkeypatch.undo()
