"""Orientation ensembles on the GPU: fd_rows_orient_f32, fd_ensemble_orient_stats_f32 and fd_rows_take_f32 at the C ABI, bit for bit
against numpy / the torch un-orient followed by metrics.ensemble_stats, and ResidualDiffusion.sample_ensemble(orientations=...) --
every replica the image a separate sample() call on the oriented slice gives, turned back; the tower once per slice and distinct
orientation; nothing dependent on the cut into passes, on the streams or on the batch -- with its callers Trainer.test and
sample_volume.  64 x 64, 2-3 DDIM steps, the tiny models of tests/test_gpu_ensemble.py."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
TINY_CLIP = dict(layers=(2, 1, 1, 1), width=16, embed_dim=1024)
D4, FLIPS = tuple(range(8)), (0, 1, 2, 3)
SHAPES = [(64, 64, D4), (72, 72, D4), (7, 7, D4), (8, 24, FLIPS)]        # one full tile; edge tiles; the scalar form; H != W


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _offset_view(t):
    """t's values in memory that starts one float past a 16-byte boundary: the kernels take their scalar path"""
    buf = torch.empty(t.numel() + 4, device=t.device, dtype=t.dtype)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def _inv(code):
    from founddiff_amd.ensemble import orientation_inverse
    return orientation_inverse(code)


def _turn(x, code):
    """the transform `code` on the last two axes of a torch tensor: rot90(flip_W(flip_H(x)), k)"""
    if code & 1:
        x = x.flip(-2)
    if code & 2:
        x = x.flip(-1)
    return torch.rot90(x, (code >> 2) & 3, (-2, -1)).contiguous()


def _i32(values):
    return torch.tensor([int(v) for v in values], dtype=torch.int32, device="cuda")


def _cycle(codes, K):
    return [codes[k % len(codes)] for k in range(K)]


# ---- fd_rows_orient_f32
def _rows_orient(src, codes, offset=False):
    from founddiff_amd import _lib as L
    B, H, W = src.shape
    K = len(codes)
    dst = torch.full((B * K, H, W), float("nan"), device="cuda")
    s = src.cuda()
    if offset:
        s, dst = _offset_view(s), _offset_view(dst)
    c = _i32(codes)
    L.call("fd_rows_orient_f32", s.data_ptr(), dst.data_ptr(), c.data_ptr(), B, K, H, W, _stream())
    return dst.view(B, K, H, W).cpu().numpy()


@pytest.mark.parametrize("H,W,codes,offset", [(64, 64, D4, False), (72, 72, D4, False), (7, 7, D4, False), (6, 6, D4, False),
                                              (8, 24, FLIPS, False), (8, 24, (8, 11, 2), True), (72, 72, D4, True),
                                              (72, 72, _cycle(D4, 9), False), (68, 68, tuple(range(16)), False)])
def test_rows_orient(H, W, codes, offset):
    from founddiff_amd.diffusion_train import augment_source_index
    src = torch.randn(2, H, W, generator=torch.Generator().manual_seed(H * 100 + W))
    got = _rows_orient(src, codes, offset)
    m = src.numpy()
    for k, c in enumerate(codes):
        i, j = augment_source_index(c, H, W)
        assert np.array_equal(got[:, k], m[:, i, j]), (k, c)


def test_rows_orient_rejects_what_the_slice_cannot_take():
    from founddiff_amd import _lib as L
    src = torch.randn(2, 8, 24).cuda()
    for codes, msg in (((0, 4), b"transposes"), ((1, 14, 2), b"transposes"), ((0, 16), b"outside 0..15"), ((-1,), b"outside 0..15")):
        dst, c = torch.full((2 * len(codes), 8, 24), 7.0, device="cuda"), _i32(codes)
        rc = L.lib().fd_rows_orient_f32(src.data_ptr(), dst.data_ptr(), c.data_ptr(), 2, len(codes), 8, 24, _stream())
        torch.cuda.synchronize()
        assert rc != 0 and msg in L.lib().fd_last_error(), codes
        assert bool((dst == 7.0).all()), codes                                # nothing was launched


# ---- fd_ensemble_orient_stats_f32
def _orient_stats(x, inv_codes, H, W, with_samples=True, offset=False):
    """x (B, K, H W), replica k read through inv_codes[k] -> mean, std (B, H W), spread (B,), samples (B, K, H W) or None"""
    from founddiff_amd import _lib as L
    B, K, n = x.shape
    mean, std = torch.full((B, n), -7.0, device="cuda"), torch.full((B, n), -7.0, device="cuda")
    out = torch.full((B, K, n), -7.0, device="cuda") if with_samples else None
    if offset:
        x, mean, std = _offset_view(x), _offset_view(mean), _offset_view(std)
        out = None if out is None else _offset_view(out)
    ws = torch.empty(B * L.lib().fd_ensemble_nblk(n), device="cuda")
    spread, c = torch.full((B,), -7.0, device="cuda"), _i32(inv_codes)
    L.call("fd_ensemble_orient_stats_f32", x.data_ptr(), c.data_ptr(), mean.data_ptr(), std.data_ptr(), ws.data_ptr(),
           spread.data_ptr(), None if out is None else out.data_ptr(), B, K, H, W, _stream())
    return mean, std, spread, out


def _composition(x, inv_codes, H, W):
    """the specification: un-orient every replica with torch, then fd_ensemble_stats_f32"""
    from founddiff_amd.metrics import ensemble_stats
    B, K, n = x.shape
    un = torch.stack([_turn(x[:, k].view(B, H, W), c) for k, c in enumerate(inv_codes)], 1).reshape(B, K, n).contiguous()
    return ensemble_stats(un) + (un,)


@pytest.mark.parametrize("K", [1, 3, 8, 9, 33])
@pytest.mark.parametrize("H,W,codes", SHAPES)
def test_orient_stats_bitwise(H, W, codes, K):
    inv = [_inv(c) for c in _cycle(codes, K)]
    x = torch.rand(2, K, H * W, generator=torch.Generator().manual_seed(K * 1000 + H)).cuda()
    ref = _composition(x, inv, H, W)
    full = _orient_stats(x, inv, H, W)
    for name, a, b in zip(("mean", "std", "spread", "samples"), full, ref):
        assert torch.equal(a, b), name
    if K == 1:
        assert not bool(full[1].any()) and not bool(full[2].any())
    bare = _orient_stats(x, inv, H, W, with_samples=False)               # the images are written only when asked for
    assert bare[3] is None
    off = _orient_stats(x, inv, H, W, offset=True)                       # the scalar form
    for name, a, b, c in zip(("mean", "std", "spread"), bare, off, ref):
        assert torch.equal(a, c) and torch.equal(b, c), name
    assert torch.equal(off[3], ref[3])


def test_orient_stats_row_independent_of_batch():
    K, H, W = 5, 72, 72
    inv = [_inv(c) for c in (5, 0, 3, 6, 4)]
    x = torch.rand(3, K, H * W, generator=torch.Generator().manual_seed(1)).cuda()
    all3 = _orient_stats(x, inv, H, W)
    for b in range(3):
        for a, one in zip(all3, _orient_stats(x[b:b + 1].contiguous(), inv, H, W)):
            assert torch.equal(a[b:b + 1], one)


def _check_stats64(x, mean, std, spread):
    """The float64 bounds of tests/test_gpu_ensemble.py, the project's number for this arithmetic.  mean: the fp32 sum of K values
    in [0, 1] in order is off by at most K^2 2^-24, the mean by K 2^-24.  std: relative 1e-4, plus what the rounded mean can add
    where the true std is about 0: at most 2 K 2^-24.  spread: relative 1e-5."""
    x64 = x.double().cpu().numpy()
    K = x64.shape[1]
    m64 = x64.mean(1)
    assert float(np.abs(mean.cpu().numpy() - m64).max()) <= K * 2.0 ** -24
    s64 = x64.std(1, ddof=1)
    assert bool((np.abs(std.cpu().numpy() - s64) <= 1e-4 * s64 + 2 * K * 2.0 ** -24).all())
    sp64 = np.sqrt((s64 ** 2).reshape(s64.shape[0], -1).mean(1))
    assert float(np.abs(spread.cpu().numpy() / sp64 - 1).max()) <= 1e-5


def test_orient_stats_vs_float64():
    K, H, W = 9, 72, 72
    inv = [_inv(c) for c in _cycle(D4, K)]
    x = torch.rand(2, K, H * W, generator=torch.Generator().manual_seed(9)).cuda()
    mean, std, spread, un = _orient_stats(x, inv, H, W)
    for k, c in enumerate(inv):                                          # the un-oriented images
        assert np.array_equal(un[:, k].view(2, H, W).cpu().numpy(), _turn(x[:, k].view(2, H, W), c).cpu().numpy())
    _check_stats64(un, mean, std, spread)


# ---- fd_rows_take_f32
@pytest.mark.parametrize("n,offset", [(4, False), (7, False), (1024, False), (1024, True)])
def test_rows_take(n, offset):
    from founddiff_amd import _lib as L
    src = torch.randn(5, n, generator=torch.Generator().manual_seed(n)).cuda()
    for idx in ([0, 0, 3, 3, 3, 1], [4, 2, 0, 3, 1], [2]):               # repeated, permuted, one row
        dst = torch.full((len(idx), n), float("nan"), device="cuda")
        s, d, rows = (_offset_view(src), _offset_view(dst), _i32(idx)) if offset else (src, dst, _i32(idx))
        L.call("fd_rows_take_f32", s.data_ptr(), d.data_ptr(), rows.data_ptr(), len(idx), n, _stream())
        assert torch.equal(d, src[idx]), idx


# ---- sample_ensemble(orientations=...)
@functools.lru_cache(maxsize=None)
def _model(ancestral=False):
    from _dist_worker import build
    return build("cuda", ancestral=ancestral)


@functools.lru_cache(maxsize=None)
def _slices(n):
    from founddiff_amd import synth
    return torch.from_numpy(synth.ct_phantom(n, 64, seed=10)[1]).cuda()


def _seeds(slice_seeds, K):
    from founddiff_amd.ensemble import ensemble_seeds
    return ensemble_seeds(slice_seeds, K)


def _stats(x):
    from founddiff_amd.metrics import ensemble_stats
    return ensemble_stats(x)


def _separate(dif, x, seeds, codes):
    """(B, K, 1, H, W): replica k of slice b as its own sample() call on the torch-oriented slice, turned back with torch"""
    K = len(codes)
    rs = _seeds(seeds, K)
    return torch.stack([torch.stack([_turn(dif.sample([_turn(x[b:b + 1], c)], batch_size=1, slice_seeds=[int(rs[b, k])])[-1],
                                           _inv(c))[0] for k, c in enumerate(codes)]) for b in range(x.shape[0])])


def _same(a, b, names=("mean", "std", "spread", "samples")):
    for name in names:
        assert torch.equal(getattr(a, name), getattr(b, name)), name


def test_d4_replicas_equal_separate_calls_ddim():
    dif, x, seeds = _model(), _slices(2), [11, 2 ** 40 + 5]
    ens = dif.sample_ensemble([x], 8, slice_seeds=seeds, return_samples=True, orientations="d4")
    assert ens.samples.shape == (2, 8, 1, 64, 64) and ens.mean.shape == (2, 1, 64, 64) and ens.spread.shape == (2,)
    ref = _separate(dif, x, seeds, D4)
    for b in range(2):
        for k in range(8):
            assert torch.equal(ens.samples[b, k], ref[b, k]), (b, k)
    mean, std, spread = _stats(ref)
    assert torch.equal(ens.mean, mean) and torch.equal(ens.std, std) and torch.equal(ens.spread, spread)
    assert float(ens.spread.min()) > 0
    # the orientation is seen by the model: replica 1 is not replica 1 of the plain ensemble
    plain = dif.sample_ensemble([x], 2, slice_seeds=seeds, return_samples=True)
    assert torch.equal(ens.samples[:, 0], plain.samples[:, 0]) and not torch.equal(ens.samples[:, 1], plain.samples[:, 1])
    # without the images: the same statistics
    bare = dif.sample_ensemble([x], 8, slice_seeds=seeds, orientations="d4")
    assert bare.samples is None
    _same(bare, ens, ("mean", "std", "spread"))


def test_replicas_equal_separate_calls_ancestral():
    dif, x = _model(ancestral=True), _slices(1)
    assert not dif.is_ddim_sampling
    ens = dif.sample_ensemble([x], 2, slice_seeds=[77], return_samples=True, orientations=(4, 3))
    ref = _separate(dif, x, [77], (4, 3))
    for k in range(2):
        assert torch.equal(ens.samples[0, k], ref[0, k]), k
    assert float(ens.std.max()) > 0


def test_k1_is_the_sample_of_the_oriented_slice_turned_back():
    dif, x = _model(), _slices(1)
    ens = dif.sample_ensemble([x], 1, slice_seeds=[12345], orientations=(5,))
    one = _turn(dif.sample([_turn(x, 5)], batch_size=1, slice_seeds=[12345])[-1], _inv(5))
    assert ens.samples is None and torch.equal(ens.mean, one)
    assert not bool(ens.std.any()) and not bool(ens.spread.any())


def test_identity_orientation_is_the_plain_ensemble():
    dif, x, seeds = _model(), _slices(2), [11, 2 ** 40 + 5]
    _same(dif.sample_ensemble([x], 3, slice_seeds=seeds, return_samples=True, orientations=(0,)),
          dif.sample_ensemble([x], 3, slice_seeds=seeds, return_samples=True))


def _count_tower_rows(monkeypatch):
    from founddiff_amd.engine import DAEngine
    rows, real = {}, DAEngine.encode_dose

    def counting(self, x_cond):
        rows[id(self)] = rows.get(id(self), 0) + x_cond.shape[0]
        return real(self, x_cond)
    monkeypatch.setattr(DAEngine, "encode_dose", counting)
    return rows


def test_tower_runs_once_per_slice_and_distinct_orientation(monkeypatch):
    dif, x = _model(), _slices(2)
    rows = _count_tower_rows(monkeypatch)
    codes = (1, 4, 1, 13)                                                # 13 is a second code of one of the 8 elements
    distinct = len({_inv(_inv(c)) for c in codes})
    assert distinct == 3
    dif.sample_ensemble([x], 5, slice_seeds=[1, 2], orientations=codes)  # 10 rows; replica 4 cycles back to code 1
    assert rows == {id(dif.model.unet0.engine()): 2 * distinct}


def test_independent_of_split_and_streams():
    dif = _model()
    saved = dif.max_sub_batch, dif.streams
    kw = dict(return_samples=True, orientations=(5, 2, 7))
    try:
        # B = 3, K = 3: passes 4 + 4 + 1 against one pass of 9
        x, seeds = _slices(3), [5, 6, 7]
        ref = dif.sample_ensemble([x], 3, slice_seeds=seeds, **kw)
        dif.max_sub_batch, dif.streams = 2, 2
        cut = dif.sample_ensemble([x], 3, slice_seeds=seeds, **kw)
        dif.max_sub_batch, dif.streams = saved
        _same(ref, cut)
        # independent of B: slice 1 alone
        one = dif.sample_ensemble([x[1:2]], 3, slice_seeds=seeds[1:2], **kw)
        for name in ("mean", "std", "spread", "samples"):
            assert torch.equal(getattr(ref, name)[1:2], getattr(one, name)), name
        # B = 2, K = 4: 8 rows on two streams against one stream
        x, seeds = _slices(2), [8, 9]
        two = dif.sample_ensemble([x], 4, slice_seeds=seeds, **kw)
        dif.streams = 1
        _same(two, dif.sample_ensemble([x], 4, slice_seeds=seeds, **kw))
    finally:
        dif.max_sub_batch, dif.streams = saved


def test_two_unets(monkeypatch):
    from founddiff_amd import arch, synth
    from founddiff_amd.DADiff import ResidualDiffusion, UnetRes, load_weights
    w = {}
    for i in (0, 1):
        w.update(synth.synth_state_dict(arch.da_unet_spec(32, (1, 2), prefix=f"model.unet{i}.", clip=TINY_CLIP), seed=i))
    net = UnetRes(dim=32, dim_mults=(1, 2), num_unet=2, condition=True, objective="pred_res_noise", test_res_or_noise="res_noise",
                  precision="fp32", clip_cfg=TINY_CLIP)
    dif = ResidualDiffusion(net, image_size=64, timesteps=1000, sampling_timesteps=2, objective="pred_res_noise", loss_type="l2",
                            condition=True, sum_scale=0.01, test_res_or_noise="res_noise")
    load_weights(dif, w)
    dif = dif.to("cuda")
    dif.init()
    x, seeds, codes = _slices(2), [21, 22], (6, 1)
    rows = _count_tower_rows(monkeypatch)
    ens = dif.sample_ensemble([x], 2, slice_seeds=seeds, return_samples=True, orientations=codes)
    assert rows == {id(dif.model.unet0.engine()): 4, id(dif.model.unet1.engine()): 4}
    ref = _separate(dif, x, seeds, codes)
    for b in range(2):
        for k in range(2):
            assert torch.equal(ens.samples[b, k], ref[b, k]), (b, k)


def test_quantiles_are_those_of_the_unoriented_images():
    from founddiff_amd.metrics import ensemble_quantiles
    dif, x = _model(), _slices(2)
    levels = (0.0, 0.5, 1.0)
    ens = dif.sample_ensemble([x], 4, slice_seeds=[3, 4], return_samples=True, quantiles=levels, orientations=(0, 5, 6, 3))
    assert ens.levels == levels and ens.quantiles.shape == (2, 3, 1, 64, 64)
    assert torch.equal(ens.quantiles, ensemble_quantiles(ens.samples, levels))
    assert torch.equal(ens.quantiles[:, 0], ens.samples.min(1).values) and torch.equal(ens.quantiles[:, 2], ens.samples.max(1).values)
    _same(ens, dif.sample_ensemble([x], 4, slice_seeds=[3, 4], return_samples=True, orientations=(0, 5, 6, 3)))


def test_trainer_test_orientations(tmp_path):
    from types import SimpleNamespace
    from founddiff_amd.DADiff import Trainer
    from founddiff_amd.data import SyntheticCTDataset
    from founddiff_amd.metrics import compute_metrics
    dif = _model()
    ds = SyntheticCTDataset(2, 64)
    tr = Trainer(SimpleNamespace(is_train=False), dif, None, num_samples=1, condition=True, num_unet=1,
                 checkpoint_folder=str(tmp_path / "ck"), is_train=False, dataset=ds)
    psnr, ssim, rmse = tr.test(n_samples=8, ensemble_seed=40, orientations="d4")
    y = torch.stack([ds[i][0] for i in range(2)]).cuda()
    x = torch.stack([ds[i][1] for i in range(2)]).cuda()
    ens = dif.sample_ensemble([x], 8, slice_seeds=[40, 41], orientations="d4")
    m = compute_metrics(ens.mean, y).cpu().numpy()
    assert np.array_equal(np.array(tr.test_running_psnr), m[:, 0]) and np.array_equal(np.array(tr.test_running_ssim), m[:, 1])
    assert np.array_equal(np.array(tr.test_running_rmse), m[:, 2])
    assert psnr == float(np.mean(m[:, 0]))
    for i in range(2):
        base = os.path.join(tr.results_folder, ds.load_name(i)[:-4])
        assert np.array_equal(np.load(base + ".npy"), ens.mean[i, 0].cpu().numpy())
        assert np.array_equal(np.load(base + "_std.npy"), ens.std[i, 0].cpu().numpy())
    # n_samples = 1: one sample of the oriented slice, turned back
    tr.test(n_samples=1, ensemble_seed=40, orientations=(6,))
    one = dif.sample_ensemble([x], 1, slice_seeds=[40, 41], orientations=(6,))
    assert np.array_equal(np.load(os.path.join(tr.results_folder, ds.load_name(1)[:-4]) + ".npy"), one.mean[1, 0].cpu().numpy())
    with pytest.raises(RuntimeError):
        tr.test(n_samples=8, orientations="d4", tile=32, tiled_ensemble=True)


def test_sample_volume_flips_on_a_wide_volume():
    """64 x 96: the U-Net is convolutional and the DA-CLIP tower pools, so the 64 x 64 model samples it"""
    from founddiff_amd import parallel
    dif, sq = _model(), _slices(3)
    vol = torch.cat([sq, sq[..., :32].flip(-1)], -1).contiguous()
    assert vol.shape == (3, 1, 64, 96)
    mean, std = parallel.sample_volume(dif, vol, noise_seed=100, batch=2, n_samples=4, orientations="flips")    # batches of 2 + 1
    ens = dif.sample_ensemble([vol], 4, slice_seeds=[100, 101, 102], return_samples=True, orientations="flips")
    assert torch.equal(mean, ens.mean) and torch.equal(std, ens.std)
    ref = _separate(dif, vol[:1], [100], FLIPS)
    assert torch.equal(ens.samples[:1], ref)
    # every rank of a world of two computes its shard alone: the shards are the rows of the whole
    for rank, sl in ((0, slice(0, 2)), (1, slice(2, 3))):
        part = dif.sample_ensemble([vol[sl]], 4, slice_seeds=[100 + i for i in range(3)][sl], orientations="flips")
        assert torch.equal(part.mean, mean[sl]) and torch.equal(part.std, std[sl]), rank
    one = parallel.sample_volume(dif, vol[:2], noise_seed=100, batch=2, n_samples=1, orientations=(2,))
    k1 = dif.sample_ensemble([vol[:2]], 1, slice_seeds=[100, 101], orientations=(2,))
    assert isinstance(one, tuple) and torch.equal(one[0], k1.mean) and not bool(one[1].any())


def test_argument_errors():
    dif, x = _model(), _slices(2)
    wide = torch.cat([x, x[..., :32]], -1).contiguous()
    with pytest.raises(RuntimeError, match="orientation ensembles of tiled samples are not built"):
        dif.sample_ensemble([x], 2, tile=32, orientations="d4")
    with pytest.raises(RuntimeError, match="flips"):
        dif.sample_ensemble([wide], 8, orientations="d4")
    with pytest.raises(RuntimeError, match="square"):
        dif.sample_ensemble([wide], 2, orientations=(0, 4))
    for bad in ((0, 16), (), "d8", (1.5,)):
        with pytest.raises(RuntimeError):
            dif.sample_ensemble([x], 2, orientations=bad)
    with pytest.raises(RuntimeError):
        dif.sample_ensemble([x], 0, orientations="d4")
    dif.input_condition = True
    try:
        with pytest.raises(RuntimeError, match="input_condition"):
            dif.sample_ensemble([x, x], 2, orientations="d4")
    finally:
        dif.input_condition = False
