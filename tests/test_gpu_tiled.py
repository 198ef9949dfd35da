"""Tiled sampling on the GPU: fd_tiles_gather_f32 and fd_tiles_blend_f32 at the C ABI against numpy indexing and a float64 blend,
and ResidualDiffusion.sample_tiled -- a one-tile plan is the slice, every tile the image a separate sample() call gives, nothing
dependent on the batch or on the cut into passes -- with its callers Trainer.test, sample_volume and Trainer.validate on centred
crops.  64 x 64 slices, tiles of 32, 3 DDIM steps, the tiny models of the other end-to-end tests.

The blend's bound, per pixel under c tiles: |out - ref| <= (2 c + 4) 2^-24 max|v|.  One rounding per product wy wx, one per fmaf and
one per den addition -- 3 c roundings, of which the c of the products and the c of the den additions act on num / den through the
weights (each at most 2^-24 relative, together below 2 c 2^-24 of a weighted mean that is at most max|v|) and the c of the fmafs are
bounded by the running |num| <= den max|v| -- plus the division's; (2 c + 4) 2^-24 max|v| covers them with the float32 weights'
own rounding (the reference uses the same float32 weights, so that part cancels)."""
import functools
import os

import numpy as np
import pytest
import torch

from test_tiling_cpu import blend64

pytestmark = pytest.mark.gpu
TINY_CLIP = dict(layers=(2, 1, 1, 1), width=16, embed_dim=1024)
# (B, H, W, th, tw, overlap, offset view): one tile; the scalar path with a 3-cover and W % 4 != 0; the 16-byte path; the 16-byte
# case on views that start one float past a 16-byte boundary
CASES = [(1, 8, 8, 8, 8, 0, False), (2, 22, 27, 8, 8, 4, False), (3, 64, 64, 32, 32, 8, False), (3, 64, 64, 32, 32, 8, True)]


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
    def __init__(self, H, W, th, tw, overlap):
        from founddiff_amd.tiling import tile_plan, tile_weights
        self.H, self.W, self.th, self.tw = H, W, th, tw
        self.ys, self.xs = tile_plan(H, th, overlap), tile_plan(W, tw, overlap)
        self.wy, self.wx = tile_weights(self.ys, H, th), tile_weights(self.xs, W, tw)
        self.my, self.mx = len(self.ys), len(self.xs)
        self.x4 = int(bool((self.xs % 4 == 0).all()))
        self.d_ys, self.d_xs = (torch.from_numpy(a.astype(np.int32)).cuda() for a in (self.ys, self.xs))
        self.d_wy, self.d_wx = torch.from_numpy(self.wy).cuda(), torch.from_numpy(self.wx).cuda()

    def gather(self, src, offset=False):
        from founddiff_amd import _lib as L
        B = src.shape[0]
        dst = torch.full((B * self.my * self.mx, self.th, self.tw), float("nan"), device="cuda")
        if offset:
            src, dst = _offset_view(src), _offset_view(dst)
        L.call("fd_tiles_gather_f32", src.data_ptr(), dst.data_ptr(), self.d_ys.data_ptr(), self.d_xs.data_ptr(), B, self.H, self.W,
               self.th, self.tw, self.my, self.mx, self.x4, _stream())
        return dst

    def blend(self, tiles, offset=False):
        from founddiff_amd import _lib as L
        B = tiles.shape[0] // (self.my * self.mx)
        out = torch.full((B, self.H, self.W), float("nan"), device="cuda")
        wx = self.d_wx
        if offset:
            tiles, out, wx = _offset_view(tiles), _offset_view(out), _offset_view(wx)
        L.call("fd_tiles_blend_f32", tiles.data_ptr(), self.d_wy.data_ptr(), wx.data_ptr(), self.d_ys.data_ptr(),
               self.d_xs.data_ptr(), out.data_ptr(), B, self.H, self.W, self.th, self.tw, self.my, self.mx, self.x4, _stream())
        return out

    def numpy_tiles(self, img):
        """[B my mx][th][tw] by numpy indexing"""
        return np.stack([img[b, y:y + self.th, x:x + self.tw] for b in range(img.shape[0]) for y in self.ys for x in self.xs])

    def check_blend(self, tiles, out):
        """out [B][H][W] against the float64 blend of tiles [B my mx][th][tw] (numpy), at the bound of the module docstring;
        pixels under one tile bit for bit"""
        T = self.my * self.mx
        for b in range(out.shape[0]):
            t = tiles[b * T:(b + 1) * T].reshape(self.my, self.mx, self.th, self.tw)
            ref = blend64(t.astype(np.float64), self.ys, self.xs, self.wy, self.wx, self.H, self.W)
            c = np.zeros((self.H, self.W))
            vmax = np.zeros((self.H, self.W))
            lone = np.zeros((self.H, self.W), dtype=np.float32)
            for iy, ya in enumerate(self.ys):
                for ix, xa in enumerate(self.xs):
                    win = (slice(ya, ya + self.th), slice(xa, xa + self.tw))
                    c[win] += 1
                    vmax[win] = np.maximum(vmax[win], np.abs(t[iy, ix]))
                    lone[win] = t[iy, ix]
            err = np.abs(out[b].astype(np.float64) - ref)
            bound = (2 * c + 4) * 2.0 ** -24 * vmax
            worst = float((err / np.maximum(bound, 1e-300)).max())
            print(f"blend {self.H}x{self.W} tile {self.th}x{self.tw} slice {b}: worst error / bound {worst:.3f}, cover up to {int(c.max())}")
            assert (err <= bound).all(), worst
            assert np.array_equal(out[b][c == 1], lone[c == 1])


@functools.lru_cache(maxsize=None)
def _plan(H, W, th, tw, overlap):
    return _Plan(H, W, th, tw, overlap)


# ---- fd_tiles_gather_f32
@pytest.mark.parametrize("B,H,W,th,tw,overlap,offset", CASES)
def test_gather(B, H, W, th, tw, overlap, offset):
    p = _plan(H, W, th, tw, overlap)
    src = torch.randn(B, H, W, generator=torch.Generator().manual_seed(H + W))
    dst = p.gather(src.cuda(), offset)
    assert np.array_equal(dst.cpu().numpy(), p.numpy_tiles(src.numpy()))


def test_three_cover_plan():
    p = _plan(22, 27, 8, 8, 4)
    assert p.ys.tolist() == [0, 4, 8, 12, 14] and p.x4 == 0 and p.mx == 6


# ---- fd_tiles_blend_f32
@pytest.mark.parametrize("B,H,W,th,tw,overlap,offset", CASES)
def test_blend_vs_float64(B, H, W, th, tw, overlap, offset):
    p = _plan(H, W, th, tw, overlap)
    tiles = torch.rand(B * p.my * p.mx, th, tw, generator=torch.Generator().manual_seed(B + H))
    out = p.blend(tiles.cuda(), offset)
    p.check_blend(tiles.numpy(), out.cpu().numpy())
    if offset:                                   # the aligned and the offset-view (scalar) forms agree bit for bit
        assert torch.equal(out, p.blend(tiles.cuda()))


@pytest.mark.parametrize("B,H,W,th,tw,overlap,offset", CASES)
def test_blend_of_a_cut_image(B, H, W, th, tw, overlap, offset):
    """tiles cut from one image blend back to it within the bound (c copies of v: the reference is v itself)"""
    p = _plan(H, W, th, tw, overlap)
    img = torch.rand(B, H, W, generator=torch.Generator().manual_seed(7 * B + W)).cuda()
    out = p.blend(p.gather(img, offset), offset)
    c = np.zeros((H, W))
    for ya in p.ys:
        for xa in p.xs:
            c[ya:ya + th, xa:xa + tw] += 1
    a, o = img.cpu().numpy().astype(np.float64), out.cpu().numpy().astype(np.float64)
    assert (np.abs(o - a) <= (2 * c + 4) * 2.0 ** -24 * np.abs(a)).all()
    assert np.array_equal(out.cpu().numpy()[:, c == 1], img.cpu().numpy()[:, c == 1])


@pytest.mark.parametrize("H,W,th,tw,overlap", [(22, 27, 8, 8, 4), (64, 64, 32, 32, 8)])
def test_blend_independent_of_batch(H, W, th, tw, overlap):
    p = _plan(H, W, th, tw, overlap)
    T = p.my * p.mx
    tiles = torch.rand(3 * T, th, tw, generator=torch.Generator().manual_seed(3)).cuda()
    all3 = p.blend(tiles)
    for b in range(3):
        assert torch.equal(all3[b:b + 1], p.blend(tiles[b * T:(b + 1) * T].clone()))


def test_kernel_shape_limits():
    from founddiff_amd import _lib as L
    p = _plan(8, 8, 8, 8, 0)
    a = torch.zeros(64, device="cuda")
    ptrs = (p.d_ys.data_ptr(), p.d_xs.data_ptr())
    for B, H, W, th, tw, my, mx in ((1, 8, 8, 9, 8, 1, 1), (1, 8, 8, 8, 9, 1, 1), (1, 8, 8, 8, 8, 0, 1), (1, 8, 8, 8, 8, 1, 0),
                                    (65536, 8, 8, 8, 8, 1, 1), (8192, 8, 8, 8, 8, 4, 2)):
        with pytest.raises(L.FoundDiffHipError, match="fd_tiles_gather_f32: unsupported shape"):
            L.call("fd_tiles_gather_f32", a.data_ptr(), a.data_ptr(), *ptrs, B, H, W, th, tw, my, mx, 1, _stream())
        with pytest.raises(L.FoundDiffHipError, match="fd_tiles_blend_f32: unsupported shape"):
            L.call("fd_tiles_blend_f32", a.data_ptr(), p.d_wy.data_ptr(), p.d_wx.data_ptr(), *ptrs, a.data_ptr(), B, H, W, th, tw,
                   my, mx, 1, _stream())
    with pytest.raises(L.FoundDiffHipError, match="null pointer"):
        L.call("fd_tiles_gather_f32", None, a.data_ptr(), *ptrs, 1, 8, 8, 8, 8, 1, 1, 1, _stream())


# ---- sample_tiled
@functools.lru_cache(maxsize=None)
def _model(ancestral=False):
    from _dist_worker import build
    return build("cuda", ancestral=ancestral)


@functools.lru_cache(maxsize=None)
def _slices(n):
    from founddiff_amd import synth
    return torch.from_numpy(synth.ct_phantom(n, 64, seed=10)[1]).cuda()


SEEDS3 = [11, 2 ** 40 + 5, 77]


def _field(dif, seeds, shape):
    return dif._keyed_noise(torch.tensor(seeds, dtype=torch.int64).cuda(), dif.X_T_STEP, shape)


@functools.lru_cache(maxsize=None)
def _tiled3(condition="tile"):
    """B = 3 at tile 32 / overlap 8 on the DDIM sampler (3 x 3 tiles per slice, origins 0, 24, 32), shared by the tests that read it"""
    return [t.clone() for t in _model().sample_tiled([_slices(3)], 32, 8, slice_seeds=SEEDS3, condition=condition)]


def test_sample_at_tile_size_is_the_same_from_capture_to_capture():
    """32 x 32 tiles put a 16 x 16 level under the tiny model, whose scans are one chunk: their carry-ins are zeroed by a kernel,
    because a memset node inside the captured loop left stale ones behind -- a row then depended on what its engine had run
    before.  Batch 4, batch 1 (another capture), batch 4 again, and the eager loop: the same bits."""
    dif = _model()
    x = _slices(4)[:, :, 16:48, 16:48].contiguous()
    seeds = [3, 4, 5, 6]
    nz = _field(dif, seeds, (4, 1, 32, 32))
    a = dif.sample([x], batch_size=4, noise=nz, slice_seeds=seeds)[-1]
    one = dif.sample([x[1:2]], batch_size=1, noise=nz[1:2], slice_seeds=seeds[1:2])[-1]
    b = dif.sample([x], batch_size=4, noise=nz, slice_seeds=seeds)[-1]
    assert torch.equal(a, b) and torch.equal(a[1:2], one)
    dif.use_graph = False
    try:
        eager = dif.sample([x], batch_size=4, noise=nz, slice_seeds=seeds)[-1]
    finally:
        dif.use_graph = True
    assert torch.equal(eager, a)


@pytest.mark.parametrize("ancestral", [False, True])
@pytest.mark.parametrize("B", [1, 2])
def test_one_tile_plan_is_the_slice(ancestral, B):
    dif, x = _model(ancestral), _slices(B)
    assert dif.is_ddim_sampling != ancestral
    seeds = SEEDS3[:B]
    ref = dif.sample([x], batch_size=B, noise=_field(dif, seeds, (B, 1, 64, 64)), slice_seeds=seeds)
    for condition in ("tile", "slice"):
        out = dif.sample_tiled([x], 64, slice_seeds=seeds, condition=condition)
        assert len(out) == 2 and out[0].shape == (B, 1, 64, 64) and out[1].shape == (B, 1, 64, 64)
        assert torch.equal(out[0], ref[0]) and torch.equal(out[1], ref[-1]), condition


def test_tiles_equal_separate_calls_and_blend():
    from founddiff_amd.tiling import tile_seeds
    dif, x = _model(), _slices(3)
    out = _tiled3()
    p = _plan(64, 64, 32, 32, 8)
    assert p.ys.tolist() == [0, 24, 32]
    b = 1
    ts = tile_seeds(SEEDS3, 9)
    field = _field(dif, SEEDS3, (3, 1, 64, 64))
    x_t, nz_t = p.gather(x[b:b + 1, 0]), p.gather(field[b:b + 1, 0])
    tiles = [dif.sample([x_t[j][None, None]], batch_size=1, noise=nz_t[j][None, None], slice_seeds=[int(ts[b, j])])[-1][0, 0]
             for j in range(9)]
    p.check_blend(torch.stack(tiles).cpu().numpy(), out[1][b].cpu().numpy())
    # the first image: x_T of the whole slice.  Three fp32 roundings on either side (normalise, axpy, unnormalise), each at most
    # 2^-24 (max|x_T| + 1), and the square root's single-precision argument: 8 of them
    x_T = (x * 2 - 1) + float(np.sqrt(dif.sum_scale)) * field
    assert float((out[0] - (x_T + 1) / 2).abs().max()) <= 8 * 2.0 ** -24 * float(x_T.abs().max() + 1)
    assert torch.equal(out[0], dif.sample([x], batch_size=3, noise=field, slice_seeds=SEEDS3)[0])


def test_ancestral_tiles_take_their_own_seeds():
    """32 x 64, two tiles of 32 x 32 without overlap: every pixel is under one tile, so the image is, bit for bit, the two batch-1
    samples under tile_seeds -- x_T from the slice's field, the step noise from the tile's own keyed stream"""
    from founddiff_amd.tiling import tile_seeds
    dif = _model(ancestral=True)
    x = _slices(1)[:, :, 16:48].contiguous()
    out = dif.sample_tiled([x], 32, 0, slice_seeds=[5])
    field = _field(dif, [5], (1, 1, 32, 64))
    ts = tile_seeds([5], 2)
    assert ts[0, 0] == 5 and ts[0, 1] != 5
    for j in range(2):
        win = (slice(None), slice(None), slice(None), slice(32 * j, 32 * j + 32))
        one = dif.sample([x[win].contiguous()], batch_size=1, noise=field[win].contiguous(), slice_seeds=[int(ts[0, j])])[-1]
        assert torch.equal(out[1][win], one), j


def test_independent_of_batch_passes_and_call():
    dif, x = _model(), _slices(3)
    ref = _tiled3()
    again = dif.sample_tiled([x], 32, 8, slice_seeds=SEEDS3)
    assert torch.equal(again[0], ref[0]) and torch.equal(again[1], ref[1])
    one = dif.sample_tiled([x[1:2]], 32, 8, slice_seeds=SEEDS3[1:2])
    assert torch.equal(one[0], ref[0][1:2]) and torch.equal(one[1], ref[1][1:2])
    saved = dif.max_sub_batch, dif.streams
    try:
        dif.max_sub_batch, dif.streams = 2, 2                 # 18 rows of two slices: passes of 4, 4, 4, 4, 2
        cut = dif.sample_tiled([x[:2]], 32, 8, slice_seeds=SEEDS3[:2])
        dif.max_sub_batch, dif.streams = 7, 1                 # 6 + 6 + 6
        cut7 = dif.sample_tiled([x[:2]], 32, 8, slice_seeds=SEEDS3[:2])
    finally:
        dif.max_sub_batch, dif.streams = saved
    for c in (cut, cut7):
        assert torch.equal(c[0], ref[0][:2]) and torch.equal(c[1], ref[1][:2])


def test_condition_slice(monkeypatch):
    from founddiff_amd.engine import DAEngine
    dif, x = _model(), _slices(3)
    tile, sl = _tiled3(), _tiled3("slice")
    assert torch.equal(sl[0], tile[0]) and not torch.equal(sl[1], tile[1])
    assert bool(torch.isfinite(sl[1]).all())
    rows, real = {}, DAEngine.encode_dose

    def counting(self, x_cond):
        rows.setdefault(id(self), []).append(tuple(x_cond.shape))
        return real(self, x_cond)
    monkeypatch.setattr(DAEngine, "encode_dose", counting)
    again = dif.sample_tiled([x], 32, 8, slice_seeds=SEEDS3, condition="slice")
    assert torch.equal(again[1], sl[1])
    # the tower ran once, on the three whole slices, on the tower-only engine
    assert rows == {id(dif.model.unet0.tower_engine()): [(3, 1, 64, 64)]}
    one = dif.sample_tiled([x[2:3]], 32, 8, slice_seeds=SEEDS3[2:3], condition="slice")
    assert torch.equal(one[1], sl[1][2:3])


def test_fp16_range_check_covers_the_tiles(golden):
    """sample()'s rule on a checkpoint whose activations leave binary16's range (tests/test_gpu_fp16.py): 'fp16' raises, 'auto'
    warns and returns the bf16 kernels' image"""
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
                dif.sample_tiled([x], 32, 8, slice_seeds=[3])
        elif prec == "auto":
            with pytest.warns(UserWarning, match="binary16"):
                outs[prec] = dif.sample_tiled([x], 32, 8, slice_seeds=[3])
            assert net.unet0.kernel_precision == "bf16"
        else:
            outs[prec] = dif.sample_tiled([x], 32, 8, slice_seeds=[3])
    assert torch.isfinite(outs["bf16"][1]).all()
    assert torch.equal(outs["auto"][1], outs["bf16"][1])


# ---- callers
def _test_trainer(folder, dif):
    from types import SimpleNamespace
    from founddiff_amd.DADiff import Trainer
    from founddiff_amd.data import SyntheticCTDataset
    ds = SyntheticCTDataset(2, 64)
    return ds, Trainer(SimpleNamespace(is_train=False), dif, None, num_samples=1, condition=True, num_unet=1,
                       checkpoint_folder=str(folder), is_train=False, dataset=ds)


def test_trainer_test_tiled(tmp_path):
    from founddiff_amd.metrics import compute_metrics
    dif = _model()
    ds, tr = _test_trainer(tmp_path / "ck", dif)
    psnr, ssim, rmse = tr.test(batch_size=2, tile=32, overlap=8, ensemble_seed=40)
    y = torch.stack([ds[i][0] for i in range(2)]).cuda()
    x = torch.stack([ds[i][1] for i in range(2)]).cuda()
    out = dif.sample_tiled([x], 32, 8, slice_seeds=[40, 41])[-1]
    m = compute_metrics(out, y).cpu().numpy()
    assert np.array_equal(np.array(tr.test_running_psnr), m[:, 0]) and np.array_equal(np.array(tr.test_running_rmse), m[:, 2])
    assert psnr == float(np.mean(m[:, 0]))
    for i in range(2):
        assert np.array_equal(np.load(os.path.join(tr.results_folder, ds.load_name(i)[:-4]) + ".npy"), out[i, 0].cpu().numpy())
    # one slice per call is still a batch of tiles: the low-latency kernel set stays off, the images are the same
    tr.test(batch_size=1, tile=32, overlap=8, ensemble_seed=40)
    assert not dif.model.unet0.low_latency and not any("ll" in k for k in dif.model.unet0._engine)
    for i in range(2):
        assert np.array_equal(np.load(os.path.join(tr.results_folder, ds.load_name(i)[:-4]) + ".npy"), out[i, 0].cpu().numpy())
    with pytest.raises(RuntimeError, match="ensembles of tiled samples"):
        tr.test(tile=32, n_samples=2)
    with pytest.raises(RuntimeError, match="last=False"):
        tr.test(tile=32, last=False)


def test_trainer_test_without_tile_is_unchanged(tmp_path):
    dif = _model()
    ds, tr = _test_trainer(tmp_path / "a", dif)
    _, tr2 = _test_trainer(tmp_path / "b", dif)
    torch.manual_seed(3)
    r1 = tr.test(batch_size=2)
    torch.manual_seed(3)
    r2 = tr2.test(batch_size=2, tile=None, overlap=0, tile_condition="tile")
    assert r1 == r2
    for i in range(2):
        name = ds.load_name(i)[:-4] + ".npy"
        a, b = (open(os.path.join(t.results_folder, name), "rb").read() for t in (tr, tr2))
        assert a == b


def test_sample_volume_tiled():
    from founddiff_amd import parallel
    dif, vol = _model(), _slices(3)
    ref = dif.sample_tiled([vol], 32, 8, slice_seeds=[100, 101, 102])[-1]
    for batch in (2, 3):                                       # batches of 2 + 1 slices, and one of 3
        out = parallel.sample_volume(dif, vol, noise_seed=100, batch=batch, tile=32, overlap=8)
        assert torch.equal(out, ref), batch
    with pytest.raises(RuntimeError, match="ensembles of tiled samples"):
        parallel.sample_volume(dif, vol, tile=32, n_samples=2)


def _val_trainer(folder, **kw):
    from test_gpu_own_train import _trainer
    from founddiff_amd.data import SyntheticCTDataset
    return _trainer(folder, 2, val_dataset=SyntheticCTDataset(3, 64, seed=11), val_bands=(0, 500, 1000), val_batch_size=8,
                    save_and_sample_every=100, **kw)


def test_validate_on_centred_crops(tmp_path):
    from founddiff_amd import diffusion_train as dt
    plain = _val_trainer(tmp_path / "a").validate()
    whole = _val_trainer(tmp_path / "b", val_crop_size=64).validate()
    assert whole == plain                                       # the whole slice as a window: the same bits
    tr = _val_trainer(tmp_path / "c", val_crop_size=(32, 48))
    res = tr.validate()
    assert res["n"] == [3, 3] and res != plain
    # eval_items on the hand-cropped tensors: origin (n - c) // 2 per axis, the draws of validate(), one batch of the 6 pairs
    ds = tr.val_dataset
    item, band, t, seeds = dt.val_draws(0, range(3), (0, 500, 1000), 1000)
    win = (slice(None), slice(None), slice(16, 48), slice(8, 56))
    nd = torch.stack([ds[int(i)][0] for i in item]).cuda()[win].contiguous()
    ld = torch.stack([ds[int(i)][1] for i in item]).cuda()[win].contiguous()
    rows = tr.model.eval_items([nd, ld], torch.from_numpy(t).cuda(), slice_seeds=torch.from_numpy(seeds).cuda())
    s = dt.val_summary(rows[0].cpu().numpy(), band, 2)
    print(f"validate() on 32 x 48 crops: loss {res['loss'][0]}, by hand {s['loss']}")
    assert res["loss"][0] == s["loss"] and res["psnr"][0] == s["psnr"] and res["rmse"][0] == s["rmse"]
    with pytest.raises(RuntimeError, match="larger than the slices"):
        _val_trainer(tmp_path / "d", val_crop_size=(64, 72)).validate()
    with pytest.raises(RuntimeError, match="val_crop_size"):
        _val_trainer(tmp_path / "e", val_crop_size=1.5)


def test_argument_errors():
    from founddiff_amd import _lib as L
    dif, x = _model(), _slices(2)
    trace, L.TRACE = L.TRACE, []
    try:
        for match, args, kw in (("multiples of 2", (31,), {}),("multiples of 2", ((32, 31),), {}), ("multiples of 2", (0,), {}),
                                ("larger than the slice", (128,), {}), ("larger than the slice", ((32, 66),), {}),
                                ("overlap", (32, 17), {}), ("overlap", (32, (8, -2)), {}), ("condition must be", (32, 8),
                                                                                            {"condition": "volume"}),
                                ("tile must be an int", (32.0,), {})):
            with pytest.raises(RuntimeError, match=match):
                dif.sample_tiled([x], *args, **kw)
        dif.input_condition = True
        try:
            with pytest.raises(RuntimeError, match="input_condition"):
                dif.sample_tiled([x, x], 32)
        finally:
            dif.input_condition = False
        assert L.TRACE == []                                    # every one of them before any launch
    finally:
        L.TRACE = trace
    with pytest.raises(ValueError):
        dif.sample_tiled([x], 32, slice_seeds=[1, 2, 3])
