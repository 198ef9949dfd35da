"""Tiled ensembles on the GPU: fd_tiles_ensemble_f32 at the C ABI, bit for bit fd_tiles_blend_f32 followed by fd_ensemble_stats_f32 and
within their float64 bounds, and ResidualDiffusion.sample_ensemble(tile=...) -- every replica the image a separate sample_tiled call
gives, the tower once per slice and tile, nothing dependent on the batch, the passes or the streams -- with its callers Trainer.test
and sample_volume.  64 x 64 slices, tiles of 32 with overlap 8 (origins 0, 24, 32: 9 tiles), 3 DDIM steps or one chunk of 50
ancestral steps, the tiny models of the other end-to-end tests.

The float64 bounds are restated from tests/test_gpu_tiled.py (the blend: (2 c + 4) 2^-24 max|v| per pixel under c tiles) and from
tests/test_gpu_ensemble.py (_check_stats64: the mean K 2^-24 for values in [0, 1]; std relative 1e-4 plus 2 K 2^-24; spread relative
1e-5)."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
TINY_CLIP = dict(layers=(2, 1, 1, 1), width=16, embed_dim=1024)
# (B, K, H, W, th, tw, oy, ox): one tile; the 16-byte form; the scalar form with lanes that straddle rows; 36 chunks, two launch_sum
# groups; a large K
KERNEL_CASES = [(1, 1, 8, 8, 8, 8, 0, 0), (2, 3, 64, 64, 32, 32, 8, 8), (1, 7, 37, 45, 16, 20, 5, 7), (1, 2, 192, 192, 64, 64, 16, 16),
                (1, 33, 64, 64, 32, 32, 8, 8)]
NAMES = ("mean", "std", "spread", "samples")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _offset_view(t):
    """t's values in memory that starts one float past a 16-byte boundary: the kernels take their scalar path"""
    buf = torch.empty(t.numel() + 4, device=t.device, dtype=t.dtype)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


class _Plan:
    def __init__(self, H, W, th, tw, oy, ox):
        from founddiff_amd.tiling import tile_plan, tile_weights
        self.H, self.W, self.th, self.tw = H, W, th, tw
        self.ys, self.xs = tile_plan(H, th, oy), tile_plan(W, tw, ox)
        self.wy, self.wx = tile_weights(self.ys, H, th), tile_weights(self.xs, W, tw)
        self.my, self.mx = len(self.ys), len(self.xs)
        self.T = self.my * self.mx
        self.x4 = int(bool((self.xs % 4 == 0).all()))
        self.d_ys, self.d_xs = (torch.from_numpy(a.astype(np.int32)).cuda() for a in (self.ys, self.xs))
        self.d_wy, self.d_wx = torch.from_numpy(self.wy).cuda(), torch.from_numpy(self.wx).cuda()

    def geom(self):
        return self.H, self.W, self.th, self.tw, self.my, self.mx, self.x4

    def blend_then_stats(self, tiles, B, K):
        """the specification: fd_tiles_blend_f32 over B K slices, then fd_ensemble_stats_f32"""
        from founddiff_amd import _lib as L
        from founddiff_amd.metrics import ensemble_stats
        samples = torch.full((B, K, self.H, self.W), float("nan"), device="cuda")
        L.call("fd_tiles_blend_f32", tiles.data_ptr(), self.d_wy.data_ptr(), self.d_wx.data_ptr(), self.d_ys.data_ptr(),
               self.d_xs.data_ptr(), samples.data_ptr(), B * K, *self.geom(), _stream())
        mean, std, spread = ensemble_stats(samples)
        return dict(mean=mean, std=std, spread=spread, samples=samples)

    def ensemble(self, tiles, B, K, want_samples=True, offset=False):
        from founddiff_amd import _lib as L
        nan = lambda *shape: torch.full(shape, float("nan"), device="cuda")
        nblk = L.lib().fd_ensemble_nblk(self.H * self.W)
        mean, std, spread, ws = nan(B, self.H, self.W), nan(B, self.H, self.W), nan(B), nan(B * nblk)
        samples = nan(B, K, self.H, self.W) if want_samples else None
        wx = self.d_wx
        if offset:
            tiles, wx, mean, std = _offset_view(tiles), _offset_view(wx), _offset_view(mean), _offset_view(std)
            samples = None if samples is None else _offset_view(samples)
        L.call("fd_tiles_ensemble_f32", tiles.data_ptr(), self.d_wy.data_ptr(), wx.data_ptr(), self.d_ys.data_ptr(),
               self.d_xs.data_ptr(), None if samples is None else samples.data_ptr(), mean.data_ptr(), std.data_ptr(), ws.data_ptr(),
               spread.data_ptr(), B, K, *self.geom(), _stream())
        return dict(mean=mean, std=std, spread=spread, samples=samples)

    def cover(self):
        c = np.zeros((self.H, self.W))
        for ya in self.ys:
            for xa in self.xs:
                c[ya:ya + self.th, xa:xa + self.tw] += 1
        return c

    def blend64(self, t):
        """(the float64 blend, max|v| over the covering tiles) of one slice's tiles t [my][mx][th][tw], with the float32 weights"""
        num, den, vmax = (np.zeros((self.H, self.W)) for _ in range(3))
        for iy, ya in enumerate(self.ys):
            for ix, xa in enumerate(self.xs):
                w = self.wy[iy].astype(np.float64)[:, None] * self.wx[ix].astype(np.float64)[None, :]
                win = (slice(ya, ya + self.th), slice(xa, xa + self.tw))
                num[win] += w * t[iy, ix]
                den[win] += w
                vmax[win] = np.maximum(vmax[win], np.abs(t[iy, ix]))
        return num / den, vmax


@functools.lru_cache(maxsize=None)
def _case(B, K, H, W, th, tw, oy, ox):
    """(plan, tiles, blend -> stats): computed once and shared by the kernel tests, which leave them unchanged"""
    p = _Plan(H, W, th, tw, oy, ox)
    tiles = torch.rand(B * K * p.T, th, tw, generator=torch.Generator().manual_seed(B + K + H)).cuda()
    return p, tiles, p.blend_then_stats(tiles, B, K)


def _same(a, b, names=NAMES):
    for name in names:
        assert a[name].shape == b[name].shape and torch.equal(a[name], b[name]), name


def _check_stats64(x, mean, std, spread):
    """tests/test_gpu_ensemble.py's float64 bounds, restated.  mean: the fp32 sum of K values in [0, 1] in order is off by at most
    K^2 2^-24, the mean by K 2^-24.  std: relative 1e-4, plus what the rounded mean can add where the true std is about 0: at most
    |m - m'| sqrt(K / (K - 1)) <= 2 K 2^-24.  spread: relative 1e-5."""
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


# ---- fd_tiles_ensemble_f32
@pytest.mark.parametrize("B,K,H,W,th,tw,oy,ox", KERNEL_CASES)
def test_kernel_is_blend_then_stats_bit_for_bit(B, K, H, W, th, tw, oy, ox):
    p, tiles, ref = _case(B, K, H, W, th, tw, oy, ox)
    out = p.ensemble(tiles, B, K)
    _same(out, ref)
    assert bool(torch.isfinite(out["samples"]).all())
    # without the images: the same statistics
    _same(p.ensemble(tiles, B, K, want_samples=False), ref, NAMES[:3])


def test_kernel_forms():
    """which case takes which form, and what it exercises"""
    p = _case(*KERNEL_CASES[1])[0]
    assert p.x4 == 1 and p.W % 4 == 0 and p.tw % 4 == 0 and p.ys.tolist() == [0, 24, 32]
    p = _case(*KERNEL_CASES[2])[0]
    assert p.W % 4 != 0 and p.x4 == 0 and p.ys.tolist() == [0, 11, 21] and p.xs.tolist() == [0, 13, 25]
    assert any((4 * g) // p.W != (4 * g + 3) // p.W for g in range(p.H * p.W // 4))        # a lane's pixels in two rows
    p = _case(*KERNEL_CASES[3])[0]
    assert -(-p.H * p.W // 1024) == 36


def test_one_tile_is_the_tile():
    p, tiles, _ = _case(*KERNEL_CASES[0])
    out = p.ensemble(tiles, 1, 1)
    assert torch.equal(out["mean"], tiles) and torch.equal(out["samples"][0], tiles)
    assert not bool(out["std"].any()) and not bool(out["spread"].any())


def test_kernel_offset_views_take_the_scalar_form_with_equal_bits():
    B, K = KERNEL_CASES[1][:2]
    p, tiles, ref = _case(*KERNEL_CASES[1])
    _same(p.ensemble(tiles, B, K, offset=True), ref)
    _same(p.ensemble(tiles, B, K, want_samples=False, offset=True), ref, NAMES[:3])


@pytest.mark.parametrize("case", [KERNEL_CASES[1], (3, 5, 37, 45, 16, 20, 5, 7)])
def test_kernel_rows_independent_of_batch(case):
    B, K = case[:2]
    p, tiles, _ = _case(*case)
    all_b = p.ensemble(tiles, B, K)
    for b in range(B):
        one = p.ensemble(tiles[b * K * p.T:(b + 1) * K * p.T].clone(), 1, K)
        for name in NAMES:
            assert torch.equal(all_b[name][b:b + 1], one[name]), (name, b)


@pytest.mark.parametrize("B,K,H,W,th,tw,oy,ox", KERNEL_CASES)
def test_kernel_vs_float64(B, K, H, W, th, tw, oy, ox):
    p, tiles, _ = _case(B, K, H, W, th, tw, oy, ox)
    out = p.ensemble(tiles, B, K)
    t = tiles.cpu().numpy().astype(np.float64).reshape(B, K, p.my, p.mx, th, tw)
    c = p.cover()
    got = out["samples"].cpu().numpy().astype(np.float64)
    worst = 0.0
    for b in range(B):
        for k in range(K):
            ref, vmax = p.blend64(t[b, k])
            err, bound = np.abs(got[b, k] - ref), (2 * c + 4) * 2.0 ** -24 * vmax
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
            assert (err <= bound).all(), (b, k, worst)
    print(f"tiles_ensemble {H}x{W} tile {th}x{tw} K={K}: worst blend error / bound {worst:.3f}, cover up to {int(c.max())}")
    flat = out["samples"].flatten(2)
    assert float(flat.min()) >= 0 and float(flat.max()) <= 1 + 2.0 ** -20          # a weighted mean of values in [0, 1]
    _check_stats64(flat, out["mean"].flatten(1), out["std"].flatten(1), out["spread"])


def test_kernel_argument_checks():
    from founddiff_amd import _lib as L
    p, tiles, _ = _case(*KERNEL_CASES[0])
    a = torch.zeros(64, device="cuda")
    ptrs = [tiles.data_ptr(), p.d_wy.data_ptr(), p.d_wx.data_ptr(), p.d_ys.data_ptr(), p.d_xs.data_ptr(), None] + [a.data_ptr()] * 4
    with pytest.raises(L.FoundDiffHipError, match="K must be at least 1"):
        L.call("fd_tiles_ensemble_f32", *ptrs, 1, 0, 8, 8, 8, 8, 1, 1, 1, _stream())
    with pytest.raises(L.FoundDiffHipError, match="fd_tiles_ensemble_f32: unsupported shape"):
        L.call("fd_tiles_ensemble_f32", *ptrs, 8192, 2, 8, 8, 8, 8, 2, 2, 1, _stream())
    with pytest.raises(L.FoundDiffHipError, match="null pointer"):
        L.call("fd_tiles_ensemble_f32", *(ptrs[:6] + [None] + ptrs[7:]), 1, 1, 8, 8, 8, 8, 1, 1, 1, _stream())


# ---- sample_ensemble(tile=...)
TILE = dict(tile=32, overlap=8)
SEEDS2 = [11, 2 ** 40 + 5]


@functools.lru_cache(maxsize=None)
def _model(ancestral=False):
    from _dist_worker import build
    dif = build("cuda", ancestral=ancestral)
    if ancestral:
        dif._anc_max_chunks = 1                                # one chunk of 50 steps of the 1000: seconds, the same code
    return dif


@functools.lru_cache(maxsize=None)
def _slices(n):
    from founddiff_amd import synth
    return torch.from_numpy(synth.ct_phantom(n, 64, seed=10)[1]).cuda()


@functools.lru_cache(maxsize=None)
def _ens(ancestral=False, fuse="final", condition="tile"):
    """B = 2, K = 3 at tile 32 / overlap 8, shared by the tests that read it"""
    return _model(ancestral).sample_ensemble([_slices(2)], 3, slice_seeds=SEEDS2, return_samples=True, tile_fuse=fuse,
                                             tile_condition=condition, **TILE)


def _equal(a, b, rows=slice(None)):
    for name in NAMES:
        assert torch.equal(getattr(a, name)[rows], getattr(b, name)), name


@pytest.mark.parametrize("ancestral", [False, True])
@pytest.mark.parametrize("fuse", ["final", "step"])
def test_replicas_equal_separate_sample_tiled_calls(fuse, ancestral):
    from founddiff_amd.ensemble import ensemble_seeds
    from founddiff_amd.metrics import ensemble_stats
    dif, x = _model(ancestral), _slices(2)
    assert dif.is_ddim_sampling != ancestral
    ens = _ens(ancestral, fuse)
    assert ens.samples.shape == (2, 3, 1, 64, 64) and ens.mean.shape == (2, 1, 64, 64) and ens.std.shape == (2, 1, 64, 64)
    assert ens.spread.shape == (2,)
    rs = ensemble_seeds(SEEDS2, 3)
    for b in range(2):
        for k in range(3):
            one = dif.sample_tiled([x[b:b + 1]], 32, 8, slice_seeds=[int(rs[b, k])], fuse=fuse)[-1]
            assert torch.equal(ens.samples[b, k], one[0]), (b, k)
    assert not torch.equal(ens.samples[0, 0], ens.samples[0, 1])
    # the statistics are those of the samples, and the replicas differ
    mean, std, spread = ensemble_stats(ens.samples)
    assert torch.equal(ens.mean, mean) and torch.equal(ens.std, std) and torch.equal(ens.spread, spread)
    assert float(ens.spread.min()) > 0
    assert not ancestral or 0 < dif._anc_steps_run <= 50      # one chunk, less what a precision tail takes over


@pytest.mark.parametrize("fuse", ["final", "step"])
def test_condition_slice_replicas(fuse):
    from founddiff_amd.ensemble import ensemble_seeds
    dif, x = _model(), _slices(2)
    ens = _ens(False, fuse, "slice")
    assert not torch.equal(ens.samples, _ens(False, fuse).samples)
    rs = ensemble_seeds(SEEDS2, 3)
    for b, k in ((0, 0), (1, 2)):
        one = dif.sample_tiled([x[b:b + 1]], 32, 8, slice_seeds=[int(rs[b, k])], condition="slice", fuse=fuse)[-1]
        assert torch.equal(ens.samples[b, k], one[0]), (b, k)


@pytest.mark.parametrize("fuse", ["final", "step"])
def test_k1_is_sample_tiled(fuse):
    dif, x = _model(), _slices(2)
    ens = dif.sample_ensemble([x], 1, slice_seeds=SEEDS2, tile_fuse=fuse, **TILE)
    ref = dif.sample_tiled([x], 32, 8, slice_seeds=SEEDS2, fuse=fuse)[-1]
    assert ens.samples is None and torch.equal(ens.mean, ref)
    assert not bool(ens.std.any()) and not bool(ens.spread.any())


def test_one_tile_plan_is_the_untiled_ensemble():
    """fuse="final": a tile row is a row of sample().  (Under "step" a one-tile plan is sample_tiled(fuse="step")'s, which has no
    precision tail on the shipped plan: the replicas test covers that contract.)"""
    dif, x = _model(), _slices(2)
    ref = dif.sample_ensemble([x], 3, slice_seeds=SEEDS2, return_samples=True)
    for condition in ("tile", "slice"):
        _equal(dif.sample_ensemble([x], 3, slice_seeds=SEEDS2, return_samples=True, tile=64, tile_condition=condition), ref)


def test_one_tile_plan_fused_is_sample_tiled_fused():
    from founddiff_amd.ensemble import ensemble_seeds
    dif, x = _model(), _slices(1)
    ens = dif.sample_ensemble([x], 2, slice_seeds=SEEDS2[:1], return_samples=True, tile=64, tile_fuse="step")
    rs = ensemble_seeds(SEEDS2[:1], 2)
    for k in range(2):
        assert torch.equal(ens.samples[0, k], dif.sample_tiled([x], 64, slice_seeds=[int(rs[0, k])], fuse="step")[-1][0]), k


def test_tile_none_is_unchanged():
    dif, x = _model(), _slices(2)
    ref = dif.sample_ensemble([x], 3, slice_seeds=SEEDS2, return_samples=True)
    _equal(dif.sample_ensemble([x], 3, slice_seeds=SEEDS2, return_samples=True, tile=None, overlap=0, tile_condition="tile",
                               tile_fuse="final"), ref)


def _count_tower_rows(monkeypatch):
    from founddiff_amd.engine import DAEngine
    rows, real = {}, DAEngine.encode_dose

    def counting(self, x_cond):
        rows[id(self)] = rows.get(id(self), 0) + x_cond.shape[0]
        return real(self, x_cond)
    monkeypatch.setattr(DAEngine, "encode_dose", counting)
    return rows


@pytest.mark.parametrize("fuse", ["final", "step"])
def test_tower_runs_once_per_slice_and_tile(monkeypatch, fuse):
    dif, x = _model(), _slices(2)
    rows = _count_tower_rows(monkeypatch)
    dif.sample_ensemble([x], 4, slice_seeds=SEEDS2, tile_fuse=fuse, **TILE)
    assert rows == {id(dif.model.unet0.engine()): 2 * 9}                      # B T tiles, not B K T
    rows.clear()
    dif.sample_ensemble([x], 4, slice_seeds=SEEDS2, tile_fuse=fuse, tile_condition="slice", **TILE)
    assert rows == {id(dif.model.unet0.tower_engine()): 2}                    # B whole slices


@pytest.mark.parametrize("fuse", ["final", "step"])
def test_independent_of_batch_split_and_streams(fuse):
    dif, x = _model(), _slices(2)
    ref = _ens(False, fuse)
    _equal(ref, dif.sample_ensemble([x[1:2]], 3, slice_seeds=SEEDS2[1:], return_samples=True, tile_fuse=fuse, **TILE), slice(1, 2))
    saved = dif.max_sub_batch, dif.streams
    try:
        dif.max_sub_batch, dif.streams = 2, 2                  # 54 rows: passes of 4 ("final"), sub-batches of 2 ("step")
        _equal(ref, dif.sample_ensemble([x], 3, slice_seeds=SEEDS2, return_samples=True, tile_fuse=fuse, **TILE))
        dif.max_sub_batch, dif.streams = saved[0], 1
        _equal(ref, dif.sample_ensemble([x], 3, slice_seeds=SEEDS2, return_samples=True, tile_fuse=fuse, **TILE))
    finally:
        dif.max_sub_batch, dif.streams = saved


@pytest.mark.parametrize("fuse", ["final", "step"])
def test_two_unets(monkeypatch, fuse):
    from founddiff_amd import arch, synth
    from founddiff_amd.DADiff import ResidualDiffusion, UnetRes, load_weights
    from founddiff_amd.ensemble import ensemble_seeds
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
    ens = dif.sample_ensemble([x], 2, slice_seeds=seeds, return_samples=True, tile_fuse=fuse, **TILE)
    assert rows == {id(dif.model.unet0.engine()): 18, id(dif.model.unet1.engine()): 18}      # once per U-Net
    rs = ensemble_seeds(seeds, 2)
    for b in range(2):
        for k in range(2):
            one = dif.sample_tiled([x[b:b + 1]], 32, 8, slice_seeds=[int(rs[b, k])], fuse=fuse)[-1]
            assert torch.equal(ens.samples[b, k], one[0]), (b, k)


def test_fp16_range_check_covers_the_replicas_tile_rows(golden):
    """sample()'s rule on a checkpoint whose activations leave binary16's range (tests/test_gpu_fp16.py: a bias scaled beyond it):
    'fp16' raises and names a replica's tile row, 'auto' warns once and returns the bf16 kernels' ensemble."""
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
            with pytest.raises(L.FoundDiffHipError, match="tile row of a replica.*binary16"):
                dif.sample_ensemble([x], 2, slice_seeds=[3], **TILE)
            with pytest.raises(L.FoundDiffHipError, match="binary16"):
                dif.sample_ensemble([x], 2, slice_seeds=[3], tile_fuse="step", **TILE)
        elif prec == "auto":
            with pytest.warns(UserWarning, match="binary16"):
                outs[prec] = dif.sample_ensemble([x], 2, slice_seeds=[3], **TILE)
            assert net.unet0.kernel_precision == "bf16"
        else:
            outs[prec] = dif.sample_ensemble([x], 2, slice_seeds=[3], **TILE)
    assert torch.isfinite(outs["bf16"].mean).all()
    assert torch.equal(outs["auto"].mean, outs["bf16"].mean) and torch.equal(outs["auto"].std, outs["bf16"].std)


def test_row_limit_and_argument_errors():
    dif, x = _model(), _slices(2)
    with pytest.raises(RuntimeError, match="more than 65535 rows"):
        dif.sample_ensemble([x[:1]], 7282, **TILE)                           # 7282 x 9 = 65538
    with pytest.raises(RuntimeError, match="n_samples must be at least 1"):
        dif.sample_ensemble([x], 0, **TILE)
    with pytest.raises(ValueError):
        dif.sample_ensemble([x], 2, slice_seeds=[1, 2, 3], **TILE)
    with pytest.raises(RuntimeError, match="tile_fuse must be 'final' or 'step'"):
        dif.sample_ensemble([x], 2, tile_fuse="each", **TILE)
    with pytest.raises(RuntimeError, match="condition must be 'tile' or 'slice'"):
        dif.sample_ensemble([x], 2, tile_condition="row", **TILE)
    with pytest.raises(RuntimeError, match="larger than the slice"):
        dif.sample_ensemble([x], 2, tile=128)
    with pytest.raises(RuntimeError, match="overlap"):
        dif.sample_ensemble([x], 2, tile=32, overlap=17)
    with pytest.raises(TypeError):
        dif.sample_ensemble([x], 2, None, False, 32)                         # keyword-only
    dif.input_condition = True
    try:
        with pytest.raises(RuntimeError, match="input_condition"):
            dif.sample_ensemble([x, x], 2, **TILE)
    finally:
        dif.input_condition = False


# ---- the callers
def test_trainer_test_tiled_ensemble(tmp_path):
    from types import SimpleNamespace
    from founddiff_amd.DADiff import Trainer
    from founddiff_amd.data import SyntheticCTDataset
    from founddiff_amd.metrics import compute_metrics
    dif = _model()
    ds = SyntheticCTDataset(2, 64)
    tr = Trainer(SimpleNamespace(is_train=False), dif, None, num_samples=1, condition=True, num_unet=1,
                 checkpoint_folder=str(tmp_path / "ck"), is_train=False, dataset=ds)
    with pytest.raises(RuntimeError, match="ensembles of tiled samples.*tiled_ensemble=True"):
        tr.test(tile=32, overlap=8, n_samples=2)
    psnr, ssim, rmse = tr.test(tile=32, overlap=8, n_samples=2, ensemble_seed=40, tiled_ensemble=True)
    assert not dif.model.unet0.low_latency and not any("ll" in k for k in dif.model.unet0._engine)
    y = torch.stack([ds[i][0] for i in range(2)]).cuda()
    x = torch.stack([ds[i][1] for i in range(2)]).cuda()
    ens = dif.sample_ensemble([x], 2, slice_seeds=[40, 41], **TILE)
    m = compute_metrics(ens.mean, y).cpu().numpy()
    assert np.array_equal(np.array(tr.test_running_psnr), m[:, 0]) and np.array_equal(np.array(tr.test_running_ssim), m[:, 1])
    assert np.array_equal(np.array(tr.test_running_rmse), m[:, 2])
    assert psnr == float(np.mean(m[:, 0]))
    for i in range(2):
        base = os.path.join(tr.results_folder, ds.load_name(i)[:-4])
        assert np.array_equal(np.load(base + ".npy"), ens.mean[i, 0].cpu().numpy())
        assert np.array_equal(np.load(base + "_std.npy"), ens.std[i, 0].cpu().numpy())
    # one slice per call, the fused mode and the slice-level tower reach sample_ensemble too
    tr.test(batch_size=1, tile=32, overlap=8, n_samples=2, ensemble_seed=40, tiled_ensemble=True, tile_fuse="step",
            tile_condition="slice")
    assert not dif.model.unet0.low_latency
    ens = dif.sample_ensemble([x], 2, slice_seeds=[40, 41], tile_fuse="step", tile_condition="slice", **TILE)
    for i in range(2):
        base = os.path.join(tr.results_folder, ds.load_name(i)[:-4])
        assert np.array_equal(np.load(base + ".npy"), ens.mean[i, 0].cpu().numpy())
        assert np.array_equal(np.load(base + "_std.npy"), ens.std[i, 0].cpu().numpy())


def test_sample_volume_tiled_ensemble():
    from founddiff_amd import parallel
    dif, vol = _model(), _slices(3)
    ens = dif.sample_ensemble([vol], 2, slice_seeds=[100, 101, 102], **TILE)
    for batch in (2, 3):                                       # batches of 2 + 1 slices, and one of 3
        mean, std = parallel.sample_volume(dif, vol, noise_seed=100, batch=batch, n_samples=2, tiled_ensemble=True, **TILE)
        assert torch.equal(mean, ens.mean) and torch.equal(std, ens.std), batch
    step = dif.sample_ensemble([vol], 2, slice_seeds=[100, 101, 102], tile_fuse="step", **TILE)
    mean, std = parallel.sample_volume(dif, vol, noise_seed=100, batch=2, n_samples=2, tiled_ensemble=True, tile_fuse="step", **TILE)
    assert torch.equal(mean, step.mean) and torch.equal(std, step.std)
    with pytest.raises(RuntimeError, match="ensembles of tiled samples.*tiled_ensemble=True"):
        parallel.sample_volume(dif, vol, n_samples=2, **TILE)
