"""Ensembles on the GPU: fd_rows_repeat_f32 and fd_ensemble_stats_f32 at the C ABI against torch / float64 numpy, and
ResidualDiffusion.sample_ensemble -- every replica the image a separate sample() call gives, the tower once per slice, nothing
dependent on the cut into passes, on the streams or on the batch -- with its callers Trainer.test and sample_volume.  64 x 64, 2-3
DDIM steps, the tiny models of the other end-to-end tests."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
TINY_CLIP = dict(layers=(2, 1, 1, 1), width=16, embed_dim=1024)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _offset_view(t):
    """t's values in memory that starts one float past a 16-byte boundary: the kernels take their scalar path"""
    buf = torch.empty(t.numel() + 4, device=t.device, dtype=t.dtype)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


# ---- fd_rows_repeat_f32
@pytest.mark.parametrize("B,K,n,offset", [(1, 1, 4, False), (3, 5, 7, False), (2, 3, 4096, False), (2, 4, 260, True)])
def test_rows_repeat(B, K, n, offset):
    from founddiff_amd import _lib as L
    src = torch.randn(B, n, generator=torch.Generator().manual_seed(B * 100 + K)).cuda()
    dst = torch.full((B * K, n), float("nan"), device="cuda")
    if offset:
        src, dst = _offset_view(src), _offset_view(dst)
    L.call("fd_rows_repeat_f32", src.data_ptr(), dst.data_ptr(), B, K, n, _stream())
    assert torch.equal(dst, src.repeat_interleave(K, 0))


# ---- fd_ensemble_stats_f32
def _stats(x):
    from founddiff_amd.metrics import ensemble_stats
    return ensemble_stats(x)


def _check_stats64(x, mean, std, spread):
    """The float64 bounds.  mean: the fp32 sum of K values in [0, 1] in order is off by at most K^2 2^-24, the mean by K 2^-24.
    std: relative 1e-4, plus what the rounded mean can add where the true std is about 0: sum (x - m')^2 = sum (x - m)^2 +
    K (m - m')^2, so at most |m - m'| sqrt(K / (K - 1)) <= 2 K 2^-24.  spread: relative 1e-5."""
    x64 = x.double().cpu().numpy()
    K = x64.shape[1]
    m64 = x64.mean(1)
    assert float(np.abs(mean.cpu().numpy() - m64).max()) <= K * 2.0 ** -24
    if K == 1:
        assert torch.equal(mean, x[:, 0]) and not bool(std.any()) and not bool(spread.any())
        return
    s64 = x64.std(1, ddof=1)
    assert bool((np.abs(std.cpu().numpy() - s64) <= 1e-4 * s64 + 2 * K * 2.0 ** -24).all())
    sp64 = np.sqrt((s64 ** 2).reshape(s64.shape[0], -1).mean(1))
    assert float(np.abs(spread.cpu().numpy() / sp64 - 1).max()) <= 1e-5


@pytest.mark.parametrize("B,K,n", [(1, 1, 16), (2, 2, 4096), (3, 7, 4099), (1, 33, 4096)])
def test_ensemble_stats_vs_float64(B, K, n):
    x = torch.rand(B, K, n, generator=torch.Generator().manual_seed(K)).cuda()
    mean, std, spread = _stats(x)
    assert mean.shape == (B, n) and std.shape == (B, n) and spread.shape == (B,)
    _check_stats64(x, mean, std, spread)
    # the aligned and the offset-view (scalar) forms agree bit for bit
    for a, b in zip((mean, std, spread), _stats(_offset_view(x))):
        assert torch.equal(a, b)


@pytest.mark.parametrize("K", [8, 33])
def test_ensemble_stats_cancellation(K):
    """x = 0.5 + 1e-3 N(0, 1): E[x^2] - mean^2 in fp32 is 40 % off here, the two-pass form 2e-7.  Every pixel is gated."""
    n = 4096
    x = torch.from_numpy((0.5 + 1e-3 * np.random.default_rng(3).standard_normal((1, K, n))).astype(np.float32)).cuda()
    s64 = x.double().cpu().numpy().std(1, ddof=1)
    assert float(s64.min()) > 2.5e-4                                          # nothing is masked
    _, std, _ = _stats(x)
    rel = float(np.abs(std.cpu().numpy() / s64 - 1).max())
    print(f"K={K}: max relative error of std {rel:.3e}")
    assert rel <= 1e-4


def test_ensemble_stats_row_independent_of_batch():
    x = torch.rand(3, 5, 4099, generator=torch.Generator().manual_seed(1)).cuda()
    all3 = _stats(x)
    for b in range(3):
        for a, one in zip(all3, _stats(x[b:b + 1])):
            assert torch.equal(a[b:b + 1], one)


# ---- sample_ensemble
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


@functools.lru_cache(maxsize=None)
def _ddim_ensemble():
    """B = 2, K = 3 on the DDIM sampler, shared by the tests that read it"""
    return _model().sample_ensemble([_slices(2)], 3, slice_seeds=[11, 2 ** 40 + 5], return_samples=True)


def test_k1_is_the_seeded_sample():
    dif, x = _model(), _slices(1)
    s = torch.tensor([12345], dtype=torch.int64)
    x_T = dif._keyed_noise(s.cuda(), dif.X_T_STEP, (1, 1, 64, 64))
    ref = dif.sample([x], batch_size=1, noise=x_T, slice_seeds=s)[-1]
    ens = dif.sample_ensemble([x], 1, slice_seeds=s)
    assert ens.samples is None and ens.mean.shape == (1, 1, 64, 64) and ens.spread.shape == (1,)
    assert torch.equal(ens.mean, ref)
    assert not bool(ens.std.any()) and not bool(ens.spread.any())


def test_replicas_equal_separate_calls_ddim():
    dif, x = _model(), _slices(2)
    ens = _ddim_ensemble()
    assert ens.samples.shape == (2, 3, 1, 64, 64)
    rs = _seeds([11, 2 ** 40 + 5], 3)
    for b in range(2):
        for k in range(3):
            one = dif.sample([x[b:b + 1]], batch_size=1, slice_seeds=[int(rs[b, k])])[-1]
            assert torch.equal(ens.samples[b, k], one[0]), (b, k)
    assert not torch.equal(ens.samples[0, 0], ens.samples[0, 1])


def test_replicas_equal_separate_calls_ancestral():
    dif, x = _model(ancestral=True), _slices(1)
    assert not dif.is_ddim_sampling
    ens = dif.sample_ensemble([x], 2, slice_seeds=[77], return_samples=True)
    rs = _seeds([77], 2)
    for k in range(2):
        one = dif.sample([x], batch_size=1, slice_seeds=[int(rs[0, k])])[-1]
        assert torch.equal(ens.samples[0, k], one[0]), k
    assert float(ens.std.max()) > 0


def test_ensemble_statistics():
    ens = _ddim_ensemble()
    mean, std, spread = _stats(ens.samples)
    assert torch.equal(ens.mean, mean) and torch.equal(ens.std, std) and torch.equal(ens.spread, spread)
    assert ens.mean.shape == (2, 1, 64, 64) and ens.std.shape == (2, 1, 64, 64) and ens.spread.shape == (2,)
    _check_stats64(ens.samples.flatten(2), ens.mean.flatten(1), ens.std.flatten(1), ens.spread)
    assert float(ens.spread.min()) > 0


def _count_tower_rows(monkeypatch):
    from founddiff_amd.engine import DAEngine
    rows, real = {}, DAEngine.encode_dose

    def counting(self, x_cond):
        rows[id(self)] = rows.get(id(self), 0) + x_cond.shape[0]
        return real(self, x_cond)
    monkeypatch.setattr(DAEngine, "encode_dose", counting)
    return rows


def test_tower_runs_once_per_slice(monkeypatch):
    dif, x = _model(), _slices(2)
    rows = _count_tower_rows(monkeypatch)
    dif.sample_ensemble([x], 4, slice_seeds=[1, 2])            # 8 rows: two streams, two engines and their tail engines
    assert rows == {id(dif.model.unet0.engine()): 2}


def test_independent_of_split_and_streams():
    dif = _model()
    saved = dif.max_sub_batch, dif.streams
    try:
        # B = 3, K = 3: passes 4 + 4 + 1 against one pass of 9
        x, seeds = _slices(3), [5, 6, 7]
        ref = dif.sample_ensemble([x], 3, slice_seeds=seeds, return_samples=True)
        dif.max_sub_batch, dif.streams = 2, 2
        cut = dif.sample_ensemble([x], 3, slice_seeds=seeds, return_samples=True)
        dif.max_sub_batch, dif.streams = saved
        for name in ("mean", "std", "spread", "samples"):
            assert torch.equal(getattr(ref, name), getattr(cut, name)), name
        # independent of B: slice 1 alone
        one = dif.sample_ensemble([x[1:2]], 3, slice_seeds=seeds[1:2], return_samples=True)
        for name in ("mean", "std", "spread", "samples"):
            assert torch.equal(getattr(ref, name)[1:2], getattr(one, name)), name
        # B = 2, K = 4: 8 rows on two streams against one stream
        x, seeds = _slices(2), [8, 9]
        two = dif.sample_ensemble([x], 4, slice_seeds=seeds, return_samples=True)
        dif.streams = 1
        one = dif.sample_ensemble([x], 4, slice_seeds=seeds, return_samples=True)
        for name in ("mean", "std", "spread", "samples"):
            assert torch.equal(getattr(two, name), getattr(one, name)), name
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
    x, seeds = _slices(2), [21, 22]
    rows = _count_tower_rows(monkeypatch)
    ens = dif.sample_ensemble([x], 2, slice_seeds=seeds, return_samples=True)
    assert rows == {id(dif.model.unet0.engine()): 2, id(dif.model.unet1.engine()): 2}
    rs = _seeds(seeds, 2)
    for b in range(2):
        for k in range(2):
            one = dif.sample([x[b:b + 1]], batch_size=1, slice_seeds=[int(rs[b, k])])[-1]
            assert torch.equal(ens.samples[b, k], one[0]), (b, k)


def test_fp16_range_check_covers_the_replicas(golden):
    """sample()'s rule on a checkpoint whose activations leave binary16's range (tests/test_gpu_fp16.py: a bias scaled beyond it):
    'fp16' raises, 'auto' warns once and returns the bf16 kernels' ensemble."""
    from founddiff_amd import _lib as L
    from founddiff_amd.DADiff import ResidualDiffusion, UnetRes
    g = golden("e2e_da_tiny")
    w = {k: v.clone() for k, v in g.weights("model.").items()}
    w["model.unet0.downs.0.0.block1.proj.bias"] += 3e5
    x = g["x_input"].cuda()[:1]
    outs = {}
    for prec in ("fp16", "bf16", "auto"):
        net = UnetRes(dim=32, dim_mults=(1, 2), num_unet=1, condition=True, objective="pred_res", test_res_or_noise="res",
                      precision=prec, clip_cfg=TINY_CLIP)
        dif = ResidualDiffusion(net, image_size=64, timesteps=1000, sampling_timesteps=2, objective="pred_res", loss_type="l2",
                                condition=True, sum_scale=0.01, test_res_or_noise="res")
        dif.load_state_dict(w, strict=False)
        dif = dif.to("cuda")
        dif.init()
        if prec == "fp16":
            with pytest.raises(L.FoundDiffHipError, match="binary16"):
                dif.sample_ensemble([x], 2, slice_seeds=[3])
        elif prec == "auto":
            with pytest.warns(UserWarning, match="binary16"):
                outs[prec] = dif.sample_ensemble([x], 2, slice_seeds=[3])
            assert net.unet0.kernel_precision == "bf16"
        else:
            outs[prec] = dif.sample_ensemble([x], 2, slice_seeds=[3])
    assert torch.isfinite(outs["bf16"].mean).all()
    assert torch.equal(outs["auto"].mean, outs["bf16"].mean) and torch.equal(outs["auto"].std, outs["bf16"].std)


def test_trainer_test_ensemble(tmp_path):
    from types import SimpleNamespace
    from founddiff_amd.DADiff import Trainer
    from founddiff_amd.data import SyntheticCTDataset
    from founddiff_amd.metrics import compute_metrics
    dif = _model()
    ds = SyntheticCTDataset(2, 64)
    tr = Trainer(SimpleNamespace(is_train=False), dif, None, num_samples=1, condition=True, num_unet=1,
                 checkpoint_folder=str(tmp_path / "ck"), is_train=False, dataset=ds)
    psnr, ssim, rmse = tr.test(n_samples=3, ensemble_seed=40)
    y = torch.stack([ds[i][0] for i in range(2)]).cuda()
    x = torch.stack([ds[i][1] for i in range(2)]).cuda()
    ens = dif.sample_ensemble([x], 3, slice_seeds=[40, 41])
    m = compute_metrics(ens.mean, y).cpu().numpy()
    assert np.array_equal(np.array(tr.test_running_psnr), m[:, 0]) and np.array_equal(np.array(tr.test_running_ssim), m[:, 1])
    assert np.array_equal(np.array(tr.test_running_rmse), m[:, 2])
    assert psnr == float(np.mean(m[:, 0]))
    for i in range(2):
        base = os.path.join(tr.results_folder, ds.load_name(i)[:-4])
        assert np.array_equal(np.load(base + ".npy"), ens.mean[i, 0].cpu().numpy())
        assert np.array_equal(np.load(base + "_std.npy"), ens.std[i, 0].cpu().numpy())
    with pytest.raises(RuntimeError):
        tr.test(n_samples=0)


def test_sample_volume_ensemble():
    from founddiff_amd import parallel
    dif, vol = _model(), _slices(3)
    mean, std = parallel.sample_volume(dif, vol, noise_seed=100, batch=2, n_samples=2)        # batches of 2 + 1 slices
    ens = dif.sample_ensemble([vol], 2, slice_seeds=[100, 101, 102])
    assert torch.equal(mean, ens.mean) and torch.equal(std, ens.std)
    a = parallel.sample_volume(dif, vol[:2], noise_seed=100, batch=2)
    b = parallel.sample_volume(dif, vol[:2], noise_seed=100, batch=2, n_samples=1)
    assert torch.is_tensor(b) and torch.equal(a, b)


def test_argument_errors():
    dif, x = _model(), _slices(2)
    with pytest.raises(RuntimeError):
        dif.sample_ensemble([x], 0)
    with pytest.raises(ValueError):
        dif.sample_ensemble([x], 2, slice_seeds=[1, 2, 3])
    dif.input_condition = True
    try:
        with pytest.raises(RuntimeError):
            dif.sample_ensemble([x, x], 2)
    finally:
        dif.input_condition = False
