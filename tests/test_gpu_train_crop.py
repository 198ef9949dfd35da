"""Random crops from a data.DeviceSliceStore (csrc/fd_train_crop.hip) on the GPU: DeviceSliceStore.batch(..., windows, crop) against
the stored slices indexed by diffusion_train.crop_source_index (which tests/test_train_crop_cpu.py holds to numpy's slice + reflect
pad + flip / rot90), the fused q_sample against the cropped batch followed by the existing q_sample, batch invariance, and
Trainer(crop_size=...).  Every comparison is bitwise: copies, or identical arithmetic.

Shapes, the smallest at which each form can go wrong (a store is a few KB):
  20 x 28 and 13 x 11 slices, crops 8 x 8, 8 x 12 (inside), 20 x 28 (the slice), 24 x 32 (padded), 23 x 31 (CW % 4 != 0: per
  pixel, odd pads), with every x0 % 4 and the extreme y0: the direct form's 4-byte aligned reads, its groups in the padding;
  72 x 72 slices, crop 68 x 68: the tiled form over one full tile and one 4 wide per axis, x0, y0 in 0..3; 68 x 68 slices, crop
  72 x 72: tiled and padded."""
import functools

import numpy as np
import pytest
import torch

from test_train_crop_cpu import codes_of, windows_of

pytestmark = pytest.mark.gpu
ND_INDEX = [0, 1, 1, 2, 0]            # 3 NDCT / 5 LD slices: items 1 and 2 (and 0 and 4) share one stored NDCT
T = 1000
CROPS = [(8, 8), (8, 12), (20, 28), (24, 32), (23, 31)]


@functools.lru_cache(maxsize=None)
def _store(H, W):
    """(store, nd, ld): random slices on the host and their store; unchanged by every test"""
    from founddiff_amd.data import DeviceSliceStore
    rng = np.random.default_rng(H * 1000 + W)
    nd, ld = rng.random((3, H, W), dtype=np.float32), rng.random((len(ND_INDEX), H, W), dtype=np.float32)
    store = DeviceSliceStore(torch.from_numpy(nd).cuda(), torch.from_numpy(ld).cuda(), ND_INDEX)
    for i in range(len(ND_INDEX)):                                       # the host copies are the stored slices
        a, b = store[i]
        assert np.array_equal(a[0].cpu().numpy(), nd[ND_INDEX[i]]) and np.array_equal(b[0].cpu().numpy(), ld[i])
    return store, nd, ld


def _expect(nd, ld, indices, codes, windows, crop):
    """store[i] indexed by crop_source_index, item by item"""
    from founddiff_amd.diffusion_train import crop_source_index
    H, W = nd.shape[1:]
    xs, xi = [], []
    for i, c, (y0, x0) in zip(indices, codes, windows):
        si, sj = crop_source_index(int(c), int(y0), int(x0), H, W, *crop)
        xs.append(nd[ND_INDEX[i]][si, sj][None])
        xi.append(ld[i][si, sj][None])
    return np.stack(xs), np.stack(xi)


def _cases(H, W, crop, codes=None):
    """every code x every window of windows_of, the items cycling through the store (every item several times)"""
    codes = codes_of(*crop) if codes is None else codes
    pairs = [(c, w) for w in windows_of(H, W, *crop) for c in codes]
    indices = [(3 * k + 1) % 5 for k in range(len(pairs))]
    return indices, [c for c, _ in pairs], [w for _, w in pairs]


def _check(store, nd, ld, indices, codes, windows, crop):
    xs, xi = store.batch(indices, codes, windows, crop)
    es, ei = _expect(nd, ld, indices, codes, windows, crop)
    assert xs.shape == xi.shape == (len(indices), 1) + tuple(crop) and xs.is_cuda
    gs, gi = xs.cpu().numpy(), xi.cpu().numpy()
    bad = [(c, w) for k, (c, w) in enumerate(zip(codes, windows)) if not (np.array_equal(gs[k], es[k]) and np.array_equal(gi[k], ei[k]))]
    assert not bad, bad[:8]


@pytest.mark.parametrize("crop", CROPS)
@pytest.mark.parametrize("H,W", [(20, 28), (13, 11)])
def test_batch_against_source_index(H, W, crop):
    """the direct and the per-pixel forms: every legal code, windows with every x0 % 4 and the extreme y0, repeated indices"""
    store, nd, ld = _store(H, W)
    if (H, W, crop) == (13, 11, (24, 32)):                               # 21 columns of padding around 11: a second reflection
        with pytest.raises(RuntimeError, match="unsupported shape"):
            store.batch([0], None, None, crop)
        return
    indices, codes, windows = _cases(H, W, crop)
    assert len(set(indices)) == 5 and len(indices) > 5
    if W - crop[1] >= 4:
        assert {x0 % 4 for _, x0 in windows} == {0, 1, 2, 3}
    _check(store, nd, ld, indices, codes, windows, crop)
    # no windows: zeros; no codes: as stored; an int is the square crop
    xs, xi = store.batch([4, 4, 0], None, None, crop)
    es, ei = _expect(nd, ld, [4, 4, 0], [0, 0, 0], [(0, 0)] * 3, crop)
    assert np.array_equal(xs.cpu().numpy(), es) and np.array_equal(xi.cpu().numpy(), ei)
    assert torch.equal(xs[0], xs[1]) and not torch.equal(xi[0], xi[2])
    if crop[0] == crop[1]:
        again = store.batch([4, 4, 0], None, None, crop[0])
        assert torch.equal(again[0], xs) and torch.equal(again[1], xi)
    if crop == (H, W):                                                   # the whole slice under code 0 is the uncropped gather
        plain = store.batch([4, 4, 0])
        assert torch.equal(plain[0], xs) and torch.equal(plain[1], xi)


def test_tiled_form_across_a_tile_edge():
    """the eight odd-k codes on a 68 x 68 crop of 72 x 72 slices (one full tile and one 4 wide per axis), x0, y0 in 0..3; then a
    72 x 72 crop of 68 x 68 slices: transposed and padded, every code"""
    store, nd, ld = _store(72, 72)
    odd = [c for c in range(16) if c & 4]
    pairs = [(c, (y0, x0)) for y0 in range(4) for x0 in range(4) for c in odd]
    indices = [(3 * k + 1) % 5 for k in range(len(pairs))]
    assert len(odd) == 8 and len(pairs) == 128
    _check(store, nd, ld, indices, [c for c, _ in pairs], [w for _, w in pairs], (68, 68))
    # both forms side by side in one call
    _check(store, nd, ld, [4, 4, 0, 2], [9, 2, 6, 13], [(3, 1), (0, 2), (1, 3), (2, 0)], (68, 68))
    small, nd, ld = _store(68, 68)
    codes = list(range(16))
    _check(small, nd, ld, [(3 * k + 1) % 5 for k in range(16)], codes, [(0, 0)] * 16, (72, 72))


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("H,W,crop", [(20, 28, (8, 12)), (72, 72, (68, 68)), (20, 28, (23, 31))])
def test_fused_equals_composed(H, W, crop, normalize):
    """q_sample(StoreBatch(..., windows, crop)) against store.batch(..., windows, crop) followed by the existing q_sample: x_in,
    x_res, noise, times and x0, with keyed noise and with given noise; a 16-byte direct shape, one with the tiled form too, and a
    per-pixel, padded one"""
    from founddiff_amd import diffusion_train as dt
    from founddiff_amd.DADiff import residual_schedule
    store, _, _ = _store(H, W)
    sch = residual_schedule(T)
    indices, codes, windows = _cases(H, W, crop)
    if H == 72:                                                          # 16 codes x 4 windows are enough of these
        keep = [k for k, (y0, x0) in enumerate(windows) if (y0, x0) in ((0, 1), (2, 2), (3, 3), (2, 0))]
        indices, codes, windows = [indices[k] for k in keep], [codes[k] for k in keep], [windows[k] for k in keep]
        assert len(keep) == 64
    B = len(indices)
    rng = np.random.default_rng(7)
    t = rng.integers(0, T, B, dtype=np.int64)
    seeds = rng.integers(0, 1 << 62, B, dtype=np.int64)
    noise = torch.randn((B, 1) + crop, generator=torch.Generator().manual_seed(3)).cuda()
    xs, xi = store.batch(indices, codes, windows, crop)
    sb = dt.StoreBatch(store, indices, codes, windows, crop)
    assert sb.shape == tuple(xs.shape)
    names = ("x_in", "x_res", "noise", "times", "x0")
    for kind, kw_dev, kw_host in (("keyed", dict(slice_seeds=torch.from_numpy(seeds).cuda(), step=11), dict(slice_seeds=seeds, step=11)),
                                  ("given", dict(noise=noise), dict(noise=noise))):
        want = dt.q_sample(xs, xi, torch.from_numpy(t).cuda(), sch, normalize=normalize, x0_out=True, **kw_dev)
        got = dt.q_sample(sb, None, t, sch, normalize=normalize, x0_out=True, **kw_host)
        assert len(got) == len(want) == 5
        bad = [n for n, g, w in zip(names, got, want) if g.shape != w.shape or not torch.equal(g, w)]
        assert not bad, (kind, bad)
        assert got[0].shape == (B, 2) + crop and torch.equal(got[4], xs * 2 - 1 if normalize else xs)
        # t and the seeds as tensors on the device give the same, and so does the four-result form
        again = dt.q_sample(sb, None, torch.from_numpy(t).cuda(), sch, normalize=normalize, **kw_dev)
        assert len(again) == 4 and all(torch.equal(g, w) for g, w in zip(again, want))
    assert not torch.equal(got[0][:, 1], (xs * 2 - 1 if normalize else xs)[:, 0])        # the batch is not degenerate
    # no windows at all: the null pointer is the window (0, 0)
    zero = dt.q_sample(dt.StoreBatch(store, indices, codes, None, crop), None, t, sch, slice_seeds=seeds, step=11, normalize=normalize)
    x0s, x0i = store.batch(indices, codes, [(0, 0)] * B, crop)
    want = dt.q_sample(x0s, x0i, torch.from_numpy(t).cuda(), sch, slice_seeds=torch.from_numpy(seeds).cuda(), step=11, normalize=normalize)
    assert all(torch.equal(g, w) for g, w in zip(zero, want))


@pytest.mark.parametrize("H,W,crop", [(20, 28, (8, 8)), (72, 72, (68, 68)), (20, 28, (23, 31))])
def test_an_item_does_not_depend_on_its_batch(H, W, crop):
    """every item alone (B = 1) gives the rows it has in the batch: the gather and the fused entry, keyed noise"""
    from founddiff_amd import diffusion_train as dt
    from founddiff_amd.DADiff import residual_schedule
    store, _, _ = _store(H, W)
    sch = residual_schedule(T)
    ws = windows_of(H, W, *crop)
    indices, codes, windows = [3, 0, 3, 4, 1], [13 if crop[0] == crop[1] else 9, 2, 6 if crop[0] == crop[1] else 3, 0, 11], \
        [ws[(7 * k + 1) % len(ws)] for k in range(5)]
    t, seeds = np.array([0, 10, 500, 998, 999]), np.array([5, 6, 7, 8, 9])
    xs, xi = store.batch(indices, codes, windows, crop)
    full = dt.q_sample(dt.StoreBatch(store, indices, codes, windows, crop), None, t, sch, slice_seeds=seeds, step=4, x0_out=True)
    for k in range(5):
        one = slice(k, k + 1)
        a, b = store.batch(indices[one], codes[one], windows[one], crop)
        assert torch.equal(a[0], xs[k]) and torch.equal(b[0], xi[k]), k
        alone = dt.q_sample(dt.StoreBatch(store, indices[one], codes[one], windows[one], crop), None, t[one], sch,
                            slice_seeds=seeds[one], step=4, x0_out=True)
        for n, g, w in zip(("x_in", "x_res", "noise", "x0"), (alone[0], alone[1], alone[2], alone[4]), (full[0], full[1], full[2], full[4])):
            assert torch.equal(g[0], w[k]), (k, n)
        assert torch.equal(alone[3][:, 0], full[3][:, k]), k


# ---- Trainer(crop_size=64, augment=True): Unet(64, (1, 2)) on 6 pairs of 80 x 96 (not square), batch 2, two micro-batches -----------
SEED, CROP, SH, SW = 5, (64, 64), 80, 96


@functools.lru_cache(maxsize=None)
def _pairs():
    rng = np.random.default_rng(21)
    return [[torch.from_numpy(rng.random((1, SH, SW), dtype=np.float32)), torch.from_numpy(rng.random((1, SH, SW), dtype=np.float32))]
            for _ in range(6)]


def _trainer(folder, steps, from_store):
    from founddiff_amd.DADiff import Trainer
    from founddiff_amd.data import DeviceSliceStore
    from test_gpu_own_train import _diffusion
    ds = _pairs()
    train = DeviceSliceStore.from_items(ds, "cuda") if from_store else ds
    return Trainer(None, _diffusion(), checkpoint_folder=str(folder), train_dataset=train, device="cuda", train_batch_size=2,
                   gradient_accumulate_every=2, save_and_sample_every=100, train_lr=1e-3, ema_update_every=1, num_samples=4,
                   train_num_steps=steps, seed=SEED, log_every=2, augment=True, crop_size=CROP[0])


_RUNS = {}


def _run(tmp_path_factory, monkeypatch, from_store, tag=""):
    """the state after two steps (every parameter, EMA and Adam tensor, as CPU tensors), the counters, the batch log, what train()
    handed to every step and the first step's loss; each run is made once"""
    from founddiff_amd import diffusion_train as dt
    from test_gpu_own_train import _state
    key = (from_store, tag)
    if key not in _RUNS:
        seen, real = [], dt.train_step

        def record(model, opt, batches, **kw):
            losses = real(model, opt, batches, **kw)
            seen.append((batches, kw, [v.clone() for v in losses]))
            return losses
        monkeypatch.setattr(dt, "train_step", record)
        tr = _trainer(tmp_path_factory.mktemp("run"), 2, from_store)
        tr.train()
        monkeypatch.undo()
        _RUNS[key] = _state(tr) + (list(tr.batch_log), seen)
    return _RUNS[key]


def _differ(a, b):
    return [k for k in a if not torch.equal(a[k], b[k])]


def test_trainer_crops_repeat(tmp_path_factory, monkeypatch):
    a, ca, la, _ = _run(tmp_path_factory, monkeypatch, True)
    b, cb, lb, _ = _run(tmp_path_factory, monkeypatch, True, "again")
    assert ca == cb and la == lb and len(la) == 4 and not _differ(a, b), _differ(a, b)[:5]


def test_trainer_draws_are_the_pure_functions(tmp_path_factory, monkeypatch):
    """the indices, windows and codes of every micro-batch equal train_batch_indices / train_crop / train_augment; the crop is
    square on non-square slices, so odd rotations are drawn"""
    from founddiff_amd import diffusion_train as dt
    _, _, log, seen = _run(tmp_path_factory, monkeypatch, True)
    assert len(seen) == 2
    odd = False
    for step, (batches, kw, _) in enumerate(seen):
        assert kw["step"] == step and len(batches) == 2 and all(isinstance(b, dt.StoreBatch) for b in batches)
        for m, sb in enumerate(batches):
            idx = dt.train_batch_indices(SEED, step, m, 2, 6, 2)
            assert log[2 * step + m] == idx and sb.indices.tolist() == idx and sb.crop == CROP and sb.shape == (2, 1) + CROP
            win = dt.train_crop(SEED, step, m, idx, SH, SW, CROP)
            assert np.array_equal(sb.windows, win) and (win[:, 0] < SH - 64).all() and (win[:, 1] < SW - 64).all()
            assert sb.codes.tolist() == dt.train_augment(SEED, step, m, idx, square=True).tolist()
            odd = odd or bool((sb.codes & 4).any())
            t, seeds = dt.train_t_and_seeds(SEED, step, m, idx, T)
            assert np.array_equal(kw["t"][m], t) and np.array_equal(kw["slice_seeds"][m], seeds)
    assert odd


def test_trainer_host_dataset_gives_the_same_bits(tmp_path_factory, monkeypatch):
    a, ca, la, sa = _run(tmp_path_factory, monkeypatch, True)
    h, ch, lh, sh = _run(tmp_path_factory, monkeypatch, False)
    assert ca == ch and la == lh and not _differ(a, h), _differ(a, h)[:5]
    assert all(torch.equal(x, y) for (_, _, p), (_, _, q) in zip(sa, sh) for x, y in zip(p, q))
    assert sh[0][0][0].indices.tolist() == [0, 1] and np.array_equal(sh[0][0][0].windows, sa[0][0][0].windows)


def test_trainer_first_loss_equals_a_manual_step(tmp_path_factory, monkeypatch, tmp_path):
    """train_step on StoreBatches built by hand from the pure functions gives the first step's loss"""
    from founddiff_amd import diffusion_train as dt
    _, _, _, seen = _run(tmp_path_factory, monkeypatch, True)
    tr = _trainer(tmp_path, 1, True)
    tr._setup_training()
    store = tr.train_dataset
    batches, ts, seeds = [], [], []
    for m in range(2):
        idx = dt.train_batch_indices(SEED, 0, m, 2, 6, 2)
        batches.append(dt.StoreBatch(store, idx, dt.train_augment(SEED, 0, m, idx), dt.train_crop(SEED, 0, m, idx, SH, SW, CROP), CROP))
        t, sd = dt.train_t_and_seeds(SEED, 0, m, idx, T)
        ts.append(t)
        seeds.append(sd)
    losses = dt.train_step(tr.model, tr.opt0, batches, t=ts, slice_seeds=seeds, step=0)
    assert len(losses) == len(seen[0][2]) == 1 and bool(torch.isfinite(losses[0]))
    assert torch.equal(losses[0], seen[0][2][0])
    print(f"[measured] first loss at crop 64 x 64 of 80 x 96: {float(losses[0]):.6f}")
