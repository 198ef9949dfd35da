"""Per-step fused tiled sampling on the GPU: fd_tiles_step_ddim_f32 / fd_tiles_step_keyed_f32 at the C ABI -- bit for bit the
composition of the existing kernels (blend the tiles' outputs to the slice, the slice-level step kernel, gather), common pixels of
overlapping tiles equal, nothing dependent on alignment, in-place or the batch, and within test_tiled_fused_cpu.fused_step64's
first-order bound of float64 -- and ResidualDiffusion.sample_tiled(fuse="step"): a one-tile plan is sample(), nothing depends on the
batch or on the cut into sub-batches, the image agrees with a tiled float64-blend oracle, Trainer.test and sample_volume pass the
argument through.  64 x 64 slices, tiles of 32 with overlap 8, the tiny models of the other end-to-end tests."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from conftest import rel_err
from test_gpu_obj_loop import SEEDS, T, _keyed, _table
from test_gpu_obj_loop import _model as _plan_model
from test_gpu_tiled import CASES, SEEDS3, _offset_view, _plan, _slices, _test_trainer
from test_tiled_fused_cpu import fused_step64

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


# ---- 1. the kernels alone
def _reads(mode):
    """(o0?, o1?, x_in?) of a mode"""
    return mode != 1, mode in (1, 2), mode != 2


def _fused(p, form, mode, o0, o1, xt, xin, par, t=0, seeds=None, offset=False, in_place=False, want_slice=True):
    """one launch of the fused step on rows [B my mx][th][tw]; returns (rows, slice image or None).  form "keyed": par the [T][8]
    table and the counter at t; "ddim": par 8 floats.  offset: every tensor on a view one float past a 16-byte boundary."""
    from founddiff_amd import _lib as L
    B = xt.shape[0] // (p.my * p.mx)
    r0, r1, ri = _reads(mode)
    o0, o1, xin = o0 if r0 else None, o1 if r1 else None, xin if ri else None
    xt = xt.clone()
    out = xt if in_place else torch.full_like(xt, float("nan"))
    sl = torch.full((B, p.H, p.W), float("nan"), device="cuda") if want_slice else None
    wx = p.d_wx
    if offset:
        o0, o1, xin, wx, sl = (None if v is None else _offset_view(v) for v in (o0, o1, xin, wx, sl))
        xt = _offset_view(xt)
        out = xt if in_place else _offset_view(out)
    geom = (p.d_wy.data_ptr(), wx.data_ptr(), p.d_ys.data_ptr(), p.d_xs.data_ptr(), B, p.H, p.W, p.th, p.tw, p.my, p.mx, p.x4)
    if form == "ddim":
        L.call("fd_tiles_step_ddim_f32", mode, _p(o0), _p(o1), xt.data_ptr(), _p(xin), par.data_ptr(), *geom, out.data_ptr(), _p(sl),
               _stream())
    else:
        t_dev = torch.tensor([t], dtype=torch.int32, device="cuda")
        L.call("fd_tiles_step_keyed_f32", mode, _p(o0), _p(o1), xt.data_ptr(), _p(xin), par.data_ptr(), t_dev.data_ptr(),
               seeds.data_ptr(), *geom, out.data_ptr(), _p(sl), T, _stream())
        torch.cuda.synchronize()
        assert int(t_dev) == t                                            # the step kernel only reads the counter
    return out, sl


def _composed(p, form, mode, o0, o1, X, XI, par, t=0, seeds=None):
    """the same step from the existing kernels: fd_tiles_blend_f32 of o0 / o1 to the slice, fd_res_step_obj_keyed (fd_res_step_obj
    step 1) on the slice.  Returns the slice image [B][H][W]."""
    from founddiff_amd import _lib as L
    B, npix = X.shape[0], p.H * p.W
    O0, O1 = p.blend(o0), p.blend(o1)
    out = torch.full_like(X, float("nan"))
    if form == "ddim":
        rows = par[None].expand(B, 8).contiguous()                # fd_res_step_obj takes a parameter row per slice
        L.call("fd_res_step_obj", mode, 1, O0.data_ptr(), O1.data_ptr(), X.data_ptr(), XI.data_ptr(), None, rows.data_ptr(), None, None,
               None, out.data_ptr(), B, npix, _stream())
        torch.cuda.synchronize()
    else:
        t_dev = torch.tensor([t], dtype=torch.int32, device="cuda")
        L.call("fd_res_step_obj_keyed", mode, O0.data_ptr(), O1.data_ptr(), X.data_ptr(), XI.data_ptr(), par.data_ptr(),
               t_dev.data_ptr(), seeds.data_ptr(), out.data_ptr(), B, npix, T, _stream())
    return out


def _ddim_par(last):
    """{ac, bc, omac, alpha, 0, 0, 0, last} at t = 666 -> 333 of the schedule sampling runs under"""
    tab = _table()
    return torch.tensor([float(tab[666, 0]), float(tab[666, 1]), float(tab[666, 2]), 0.0 if last else float(tab[666, 0] - tab[333, 0]),
                         0.0, 0.0, 0.0, float(last)], dtype=torch.float32).cuda()


FORMS = [("keyed", 0), ("keyed", 1), ("keyed", 999), ("ddim", 0), ("ddim", 1)]          # (form, t or `last`)


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("B,H,W,th,tw,overlap,offset", CASES)
def test_step_kernels(B, H, W, th, tw, overlap, offset, mode):
    """Both entry points on a plan of test_gpu_tiled.CASES, the keyed form with the counter at 0, 1 and 999 and the DDIM form before
    and on the last step; x_t and x_in are rows gathered from slice-level tensors.

    The float64 gate is fused_step64's: test_gpu_obj_loop._ref64's first-order bound with the blend's (2 c + 4) 2^-24 max|v| per
    blended stream (c covering tiles) carried through the mode's formulas (tests/test_tiled_fused_cpu.py).  Observed on the MI355X:
    DESIGN.md section 4."""
    p = _plan(H, W, th, tw, overlap)
    R = B * p.my * p.mx
    g = torch.Generator().manual_seed(1000 + 10 * H + mode)
    o0, o1 = (torch.randn(R, th, tw, generator=g).cuda() for _ in range(2))
    X = (torch.randn(B, H, W, generator=g) * 0.6).cuda()
    XI = (torch.rand(B, H, W, generator=g) * 2 - 1).cuda()
    xt, xin = p.gather(X), p.gather(XI)
    seeds = torch.tensor(SEEDS[:B], dtype=torch.int64).cuda()
    keyed_tab = _table().cuda()
    f64 = lambda v: v.double().cpu().numpy()
    worst = 0.0
    for form, k in FORMS:
        par, t = (keyed_tab, k) if form == "keyed" else (_ddim_par(k), 0)
        rows, sl = _fused(p, form, mode, o0, o1, xt, xin, par, t, seeds, offset)
        # bit for bit the existing kernels' composition, on the rows and on the slice image
        want = _composed(p, form, mode, o0, o1, X, XI, par, t, seeds)
        assert torch.equal(sl, want), (form, k)
        assert torch.equal(rows, p.gather(want)), (form, k)
        # common pixels of overlapping tiles are equal: every covering tile holds the slice's value
        assert torch.equal(rows, p.gather(sl.contiguous())), (form, k)
        # the same bits aligned or not, in place, without the slice output, and for a slice alone
        if offset:
            assert torch.equal(_fused(p, form, mode, o0, o1, xt, xin, par, t, seeds)[0], rows), (form, k)
        inp, _ = _fused(p, form, mode, o0, o1, xt, xin, par, t, seeds, offset, in_place=True, want_slice=False)
        assert torch.equal(inp, rows), (form, k)
        n = p.my * p.mx
        for b in range(1, B):
            one = slice(b * n, (b + 1) * n)
            r1, s1 = _fused(p, form, mode, o0[one].contiguous(), o1[one].contiguous(), xt[one].contiguous(), xin[one].contiguous(), par,
                            t, seeds[b:b + 1].contiguous(), offset)
            assert torch.equal(r1, rows[one]) and torch.equal(s1[0], sl[b]), (form, k, b)
        # float64
        z = f64(_keyed(seeds, t, B, H * W)).reshape(B, H, W) if form == "keyed" else None
        shape = (p.my, p.mx, th, tw)
        for b in range(B):
            one = slice(b * n, (b + 1) * n)
            ref, bound, ref_sl = fused_step64(mode, form, f64(o0[one]).reshape(shape), f64(o1[one]).reshape(shape),
                                              f64(xt[one]).reshape(shape), f64(xin[one]).reshape(shape), f64(par[t] if form == "keyed" else par),
                                              p.ys, p.xs, p.wy, p.wx, H, W, None if z is None else z[b], t)
            err = np.abs(f64(rows[one]).reshape(shape) - ref)
            ratio = float((err / np.maximum(bound, 1e-300)).max())
            worst = max(worst, ratio)
            assert np.isfinite(f64(rows[one])).all() and bool((err <= bound).all()), (form, k, b, float(err.max()), ratio)
            assert bool((np.abs(f64(sl[b]) - ref_sl) <= 1e-5 + np.abs(ref_sl) * 1e-5).all())       # the assembly: every pixel from its first cover
        print(f"[measured] fd_tiles_step_{form}_f32 mode {mode} {H}x{W} tile {th}x{tw} offset {offset} "
              f"{'t' if form == 'keyed' else 'last'} {k}: worst err / bound so far {worst:.3f}")
    assert worst <= 1.0


def test_keyed_noise_is_the_slices():
    """another slice seed: another image at t > 0, the same at t = 0"""
    p = _plan(22, 27, 8, 8, 4)
    R = 2 * p.my * p.mx
    g = torch.Generator().manual_seed(5)
    o0, o1 = (torch.randn(R, 8, 8, generator=g).cuda() for _ in range(2))
    xt, xin = p.gather(torch.randn(2, 22, 27, generator=g).cuda()), p.gather(torch.rand(2, 22, 27, generator=g).cuda())
    tab = _table().cuda()
    a, b = (torch.tensor(s, dtype=torch.int64).cuda() for s in (SEEDS[:2], [s + 1 for s in SEEDS[:2]]))
    assert torch.equal(_fused(p, "keyed", 2, o0, o1, xt, xin, tab, 0, a)[0], _fused(p, "keyed", 2, o0, o1, xt, xin, tab, 0, b)[0])
    assert not torch.equal(_fused(p, "keyed", 2, o0, o1, xt, xin, tab, 17, a)[0], _fused(p, "keyed", 2, o0, o1, xt, xin, tab, 17, b)[0])


def test_kernel_argument_checks():
    from founddiff_amd import _lib as L
    p = _plan(8, 8, 8, 8, 0)
    a = torch.zeros(64, device="cuda")
    par = torch.zeros(8, device="cuda")
    t_dev, seeds = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    w = (p.d_wy.data_ptr(), p.d_wx.data_ptr(), p.d_ys.data_ptr(), p.d_xs.data_ptr())
    A = a.data_ptr()
    for B, H, W, th, tw, my, mx in ((1, 8, 8, 9, 8, 1, 1), (1, 8, 8, 8, 9, 1, 1), (1, 8, 8, 8, 8, 0, 1), (1, 8, 8, 8, 8, 1, 0),
                                    (65536, 8, 8, 8, 8, 1, 1), (8192, 8, 8, 8, 8, 4, 2)):
        with pytest.raises(L.FoundDiffHipError, match="fd_tiles_step_ddim_f32: unsupported shape"):
            L.call("fd_tiles_step_ddim_f32", 0, A, None, A, A, par.data_ptr(), *w, B, H, W, th, tw, my, mx, 1, A, None, _stream())
        with pytest.raises(L.FoundDiffHipError, match="fd_tiles_step_keyed_f32: unsupported shape"):
            L.call("fd_tiles_step_keyed_f32", 0, A, None, A, A, par.data_ptr(), t_dev.data_ptr(), seeds.data_ptr(), *w, B, H, W, th, tw,
                   my, mx, 1, A, None, T, _stream())
    ok = (1, 8, 8, 8, 8, 1, 1, 1)
    with pytest.raises(L.FoundDiffHipError, match="null pointer"):
        L.call("fd_tiles_step_ddim_f32", 0, A, None, None, A, par.data_ptr(), *w, *ok, A, None, _stream())
    with pytest.raises(L.FoundDiffHipError, match="null pointer"):
        L.call("fd_tiles_step_keyed_f32", 0, A, None, A, A, par.data_ptr(), None, seeds.data_ptr(), *w, *ok, A, None, T, _stream())
    with pytest.raises(L.FoundDiffHipError, match="mode 2 needs"):
        L.call("fd_tiles_step_ddim_f32", 2, A, None, A, A, par.data_ptr(), *w, *ok, A, None, _stream())
    with pytest.raises(L.FoundDiffHipError, match="bad mode"):
        L.call("fd_tiles_step_keyed_f32", 4, A, A, A, A, par.data_ptr(), t_dev.data_ptr(), seeds.data_ptr(), *w, *ok, A, None, T, _stream())


# ---- 2. sample_tiled(fuse="step")
def _field(dif, seeds, shape):
    return dif._keyed_noise(torch.tensor(seeds, dtype=torch.int64).cuda(), dif.X_T_STEP, shape)


@pytest.mark.parametrize("ancestral", [False, True])
@pytest.mark.parametrize("name", ["pred_noise", "res_noise"])
def test_one_tile_plan_is_sample(name, ancestral):
    """tile 64 on a 64 x 64 slice: the fused loop is sample() bit for bit -- the one-U-Net pred_noise model and the two-U-Net
    res_noise model, 4-step DDIM and the ancestral sampler bounded to one chunk of 50 steps, both values of `condition`"""
    dif = _plan_model(name, T if ancestral else 4)
    if ancestral:
        dif._anc_max_chunks = 1
    x, seeds = _slices(2), SEEDS3[:2]
    ref = dif.sample([x], batch_size=2, noise=_field(dif, seeds, (2, 1, 64, 64)), slice_seeds=seeds)
    assert not ancestral or dif._anc_steps_run == 50
    for condition in ("tile", "slice"):
        dif._anc_steps_run = None
        out = dif.sample_tiled([x], 64, slice_seeds=seeds, condition=condition, fuse="step")
        assert len(out) == 2 and out[1].shape == (2, 1, 64, 64)
        assert torch.equal(out[0], ref[0]) and torch.equal(out[1], ref[-1]), condition
        assert not ancestral or dif._anc_steps_run == 50
    assert bool(torch.isfinite(ref[-1]).all()) and not torch.equal(ref[-1], ref[0])


@functools.lru_cache(maxsize=None)
def _shipped():
    from test_gpu_tiled import _model
    return _model()


def test_repeatable_and_independent_of_the_cut():
    """tile 32 / overlap 8 (origins 0, 24, 32: 9 tiles per slice) on B = 3, the shipped bf16 model, 3 DDIM steps"""
    dif, x = _shipped(), _slices(3)
    ref = dif.sample_tiled([x], 32, 8, slice_seeds=SEEDS3, fuse="step")
    again = dif.sample_tiled([x], 32, 8, slice_seeds=SEEDS3, fuse="step")
    assert torch.equal(again[0], ref[0]) and torch.equal(again[1], ref[1])
    one = dif.sample_tiled([x[1:2]], 32, 8, slice_seeds=SEEDS3[1:2], fuse="step")
    assert torch.equal(one[0], ref[0][1:2]) and torch.equal(one[1], ref[1][1:2])
    saved = dif.max_sub_batch, dif.streams
    try:
        for cut in ((2, 2), (7, 1)):                              # 27 rows in sub-batches of 2 (the last one 1), and of 7 (the last one 6)
            dif.max_sub_batch, dif.streams = cut
            c = dif.sample_tiled([x], 32, 8, slice_seeds=SEEDS3, fuse="step")
            assert torch.equal(c[0], ref[0]) and torch.equal(c[1], ref[1]), cut
    finally:
        dif.max_sub_batch, dif.streams = saved
    final = dif.sample_tiled([x], 32, 8, slice_seeds=SEEDS3)
    assert torch.equal(ref[0], final[0]) and not torch.equal(ref[1], final[1])
    assert bool(torch.isfinite(ref[1]).all())
    sl = dif.sample_tiled([x], 32, 8, slice_seeds=SEEDS3, condition="slice", fuse="step")
    assert torch.equal(sl[0], ref[0]) and not torch.equal(sl[1], ref[1]) and bool(torch.isfinite(sl[1]).all())


def test_ancestral_two_unet_tiles():
    """the keyed form in the loop on more than one tile: the two-U-Net res_noise model, one chunk of the ancestral sampler, B = 2;
    repeatable, a slice alone has its bits, finite"""
    dif = _plan_model("res_noise", T)
    dif._anc_max_chunks = 1
    x, seeds = _slices(2), SEEDS3[:2]
    a = dif.sample_tiled([x], 32, 8, slice_seeds=seeds, fuse="step")
    assert dif._anc_steps_run == 50 and bool(torch.isfinite(a[1]).all()) and not torch.equal(a[1], a[0])
    one = dif.sample_tiled([x[1:2]], 32, 8, slice_seeds=seeds[1:2], fuse="step")
    assert torch.equal(one[1], a[1][1:2])
    other = dif.sample_tiled([x[1:2]], 32, 8, slice_seeds=[seeds[1] + 1], fuse="step")
    assert not torch.equal(other[1], one[1])


def test_against_the_tiled_oracle():
    """The shipped plan, precision="fp32", 3 DDIM steps, B = 1, tile 32 / overlap 8, against oracle.sampler.ResidualOracle with
    model_outputs cut into the plan's tiles -- every tile evaluated under its own conditioning, the raw outputs blended in float64
    -- at the project's fp32 gate, 1e-3 of max|ref|.  Measured on the MI355X: DESIGN.md section 4."""
    sys.path.insert(0, ROOT)
    from founddiff_amd import arch, synth
    from founddiff_amd.DADiff import ResidualDiffusion, UnetRes, load_weights
    from oracle import sampler
    from test_gpu_tiled import TINY_CLIP
    from test_tiling_cpu import blend64
    w = synth.synth_state_dict(arch.da_unet_spec(32, (1, 2), prefix="model.unet0.", clip=TINY_CLIP), seed=0)
    net = UnetRes(dim=32, dim_mults=(1, 2), num_unet=1, condition=True, objective="pred_res", test_res_or_noise="res", precision="fp32",
                  clip_cfg=TINY_CLIP)
    dif = ResidualDiffusion(net, image_size=64, timesteps=T, sampling_timesteps=3, objective="pred_res", loss_type="l2", condition=True,
                            sum_scale=0.01, test_res_or_noise="res")
    load_weights(dif, w)
    dif = dif.to("cuda")
    dif.init()
    p = _plan(64, 64, 32, 32, 8)
    x, seeds = _slices(1), [SEEDS3[1]]
    out = dif.sample_tiled([x], 32, 8, slice_seeds=seeds, fuse="step")

    class TiledOracle(sampler.ResidualOracle):
        def model_outputs(self, x_in, x_t, t_idx):
            cut = lambda a: torch.stack([a[0, :, y:y + p.th, xa:xa + p.tw] for y in p.ys for xa in p.xs])
            o0, _ = super().model_outputs(cut(x_in), cut(x_t), t_idx.expand(p.my * p.mx))      # the tower sees every tile's own x_in
            tiles = o0[:, 0].double().numpy().reshape(p.my, p.mx, p.th, p.tw)
            return torch.from_numpy(blend64(tiles, p.ys, p.xs, p.wy, p.wx, p.H, p.W)).float()[None, None], None
    ref = TiledOracle(w, prefix="model.unet0.", sampling_timesteps=3).sample(x.cpu(), _field(dif, seeds, (1, 1, 64, 64)).cpu())
    e0, e1 = rel_err(out[0].cpu(), ref[0]), rel_err(out[1].cpu(), ref[-1])
    print(f"[measured] sample_tiled(fuse='step') fp32 against the tiled oracle: x_T {e0:.3e}, final image {e1:.3e} of max|ref|")
    assert e0 < 1e-5 and e1 < 1e-3
    plain = sampler.ResidualOracle(w, prefix="model.unet0.", sampling_timesteps=3).sample(x.cpu(), _field(dif, seeds, (1, 1, 64, 64)).cpu())
    assert rel_err(plain[-1], ref[-1]) > 1e-3                    # the windowed model is another model: the oracle had to be tiled


def test_trainer_and_volume_pass_the_argument_through(tmp_path):
    from founddiff_amd import parallel
    dif = _shipped()
    ds, tr = _test_trainer(tmp_path / "ck", dif)
    tr.test(batch_size=2, tile=32, overlap=8, ensemble_seed=40, tile_fuse="step")
    x = torch.stack([ds[i][1] for i in range(2)]).cuda()
    out = dif.sample_tiled([x], 32, 8, slice_seeds=[40, 41], fuse="step")[-1]
    final = dif.sample_tiled([x], 32, 8, slice_seeds=[40, 41])[-1]
    assert not torch.equal(out, final)
    for i in range(2):
        assert np.array_equal(np.load(os.path.join(tr.results_folder, ds.load_name(i)[:-4]) + ".npy"), out[i, 0].cpu().numpy())
    vol = _slices(3)
    ref = dif.sample_tiled([vol], 32, 8, slice_seeds=[100, 101, 102], fuse="step")[-1]
    for batch in (2, 3):
        assert torch.equal(parallel.sample_volume(dif, vol, noise_seed=100, batch=batch, tile=32, overlap=8, tile_fuse="step"), ref), batch


def test_argument_errors():
    from founddiff_amd import _lib as L
    dif, x = _shipped(), _slices(2)
    trace, L.TRACE = L.TRACE, []
    try:
        with pytest.raises(RuntimeError, match="fuse must be"):
            dif.sample_tiled([x], 32, 8, fuse="each")
        dif.input_condition = True
        try:
            with pytest.raises(RuntimeError, match="input_condition"):
                dif.sample_tiled([x, x], 32, fuse="step")
        finally:
            dif.input_condition = False
        with pytest.raises(RuntimeError, match="larger than the slice"):
            dif.sample_tiled([x], 128, fuse="step")
        assert L.TRACE == []                                    # every one of them before any launch
    finally:
        L.TRACE = trace
