"""Calibrated intervals on the GPU: fd_interval_hist_f32 against the numpy oracle of tests/interval_cases.py, counts exactly equal --
every shape edge, the 16-byte and the scalar form, maps inside a quantile tensor, planted scores on grid values, NaN and inf pixels,
the air slice -- fd_interval_scale_f32 bit for bit against numpy float32 with its width, the two kernels against each other, and
Trainer.calibrate_intervals / Trainer.test(interval_scale=...) end to end on the 64 x 64 tiny model of the other end-to-end tests."""
import functools
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

import interval_cases as ic

pytestmark = pytest.mark.gpu
NS = (4, 7, 1024 + 7, 4096, 72 * 72)              # one vector; less than two; a partly filled second block; full blocks; several + a tail
BS = (1, 3)
SCALES = (0.0, 1.0, 1.53125, 16.0)


def _offset_view(t):
    """t's values in memory that starts one float past a 16-byte boundary: the kernels take their scalar path"""
    buf = torch.empty(t.numel() + 4, device=t.device, dtype=t.dtype)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


@functools.lru_cache(maxsize=None)
def _case(B, n, G):
    """(the four maps as numpy (B, n) with NaNs planted in each map in turn, the same on the device): computed once, left unchanged"""
    maps = list(ic.planted_maps(B, n, ic.GRIDS[G], seed=100 * n + 10 * G + B))
    if n >= 1024:
        for which in range(4):
            maps[which][B - 1, 5 + which] = np.nan
            maps[which][0, n - 1 - which] = np.nan
    else:
        maps[(n + B) % 4][B - 1, n - 1] = np.nan
    return tuple(maps), tuple(torch.from_numpy(v).cuda() for v in maps)


def _hist(dev_maps, grid, offset=False):
    from founddiff_amd.metrics import interval_hist
    if offset:
        dev_maps = [_offset_view(t) for t in dev_maps]
    else:
        assert all(t.data_ptr() % 16 == 0 for t in dev_maps)
    return interval_hist(*dev_maps, grid).cpu().numpy()


# ---- fd_interval_hist_f32
@pytest.mark.parametrize("G", [1, 2, 33, 4096])
def test_hist_counts_exactly(G):
    grid = ic.GRIDS[G]
    for B in BS:
        for n in NS:
            maps, dev = _case(B, n, G)
            want = ic.hist(*maps, grid)
            assert want.shape == (B, G + 1) and (want.sum(1) == n).all()
            if n >= 1024:
                assert (want[:, G] >= 2).any() and want[:, :G].sum() > 0         # NaN / inf pixels, and covered ones
            for offset in (False, True):
                got = _hist(dev, grid, offset)
                assert got.dtype == np.int64 and got.shape == (B, G + 1)
                assert (got.sum(1) == n).all(), (B, n, offset)
                assert np.array_equal(got, want), (B, n, offset, np.argwhere(got != want)[:4])


@pytest.mark.parametrize("n", [7, 4096])
def test_hist_of_maps_inside_a_quantile_tensor(n):
    """lo and hi as rows 0 and Q - 1 of one (B, Q, n) tensor: batch stride Q n, a multiple of 4 at n = 4096 and not at n = 7"""
    from founddiff_amd import _lib as L
    from founddiff_amd.metrics import interval_hist
    B, Q, G = 3, 3, 33
    grid = ic.GRIDS[G]
    maps, dev = _case(B, n, G)
    q = torch.zeros(B, Q, n, device="cuda")
    q[:, 0], q[:, Q - 1] = dev[1], dev[2]
    lo, hi = q[:, 0], q[:, Q - 1]
    assert not lo.is_contiguous() and lo.stride(0) == Q * n and ((Q * n) % 4 == 0) == (n == 4096)
    want = ic.hist(*maps, grid)
    assert np.array_equal(interval_hist(dev[0], lo, hi, dev[3], grid).cpu().numpy(), want)
    # the same at the C ABI, on the strides themselves
    nblk = L.lib().fd_interval_hist_nblk(n)
    ws = torch.empty(B * nblk * (G + 1), device="cuda", dtype=torch.int32)
    out = torch.full((B, G + 1), -1, device="cuda", dtype=torch.int64)
    g_dev = torch.from_numpy(grid).cuda()
    L.call("fd_interval_hist_f32", dev[0].data_ptr(), n, lo.data_ptr(), Q * n, hi.data_ptr(), Q * n, dev[3].data_ptr(), n,
           g_dev.data_ptr(), G, 1 / 3000, ws.data_ptr(), out.data_ptr(), B, n, torch.cuda.current_stream().cuda_stream)
    assert np.array_equal(out.cpu().numpy(), want)


def test_hist_rows_are_independent_of_the_batch():
    for G in (2, 4096):
        for n in (1024 + 7, 72 * 72):
            _, dev = _case(3, n, G)
            full = _hist(dev, ic.GRIDS[G])
            for b in range(3):
                alone = _hist([t[b:b + 1].clone() for t in dev], ic.GRIDS[G])
                assert np.array_equal(alone, full[b:b + 1]), (G, n, b)


@pytest.mark.parametrize("size", [64, 256])
def test_air_slices_and_the_last_finite_bin(size):
    """all four maps zero: every pixel has s = 0 and sits in bin 0, one counter for the whole slice; and every pixel on the last
    grid value: bin G - 1"""
    from founddiff_amd.metrics import interval_hist
    n = size * size
    z = torch.zeros(2, 1, size, size, device="cuda")
    for G in (1, 33, 4096):
        h = interval_hist(z, z, z, z, ic.GRIDS[G]).cpu().numpy()
        assert h.shape == (2, G + 1) and (h[:, 0] == n).all() and h.sum() == 2 * n, G
        top = float(ic.GRIDS[G][-1])
        m, l, u = (torch.full_like(z, v) for v in (0.5, 0.375, 0.75))
        h = interval_hist(m, l, u, torch.full_like(z, 0.5 + top * 0.25), ic.GRIDS[G]).cpu().numpy()
        assert (h[:, G - 1] == n).all() and h.sum() == 2 * n, G
    # half air, half tissue inside one wave's pixels: both common bins are settled by ballot
    y = z.clone()
    y[..., 1::2] = 0.002
    h = interval_hist(z, z, z, y, ic.GRIDS[33]).cpu().numpy()
    want = ic.hist(*(t.cpu().numpy().reshape(2, n) for t in (z, z, z, y)), ic.GRIDS[33])
    assert np.array_equal(h, want) and (h[:, 0] == n // 2).all()


# ---- fd_interval_scale_f32
def _scale(dev_maps, scale, offset=False):
    from founddiff_amd.metrics import interval_scale
    if offset:
        dev_maps = [_offset_view(t) for t in dev_maps]
    return interval_scale(*dev_maps, scale)


@pytest.mark.parametrize("scale", SCALES)
def test_scaled_maps_bit_for_bit_and_the_width(scale):
    """lo_out, hi_out: the bits of numpy float32.  width within n 2^-24 max|hi_out - lo_out| of the float64 mean (the first-order
    bound of an fp32 sum of n terms), the same bits in both access forms and alone."""
    for B in BS:
        for n in NS:
            maps, dev = _case(B, n, 33)
            clean = [np.where(np.isnan(v), np.float32(0.5), v) for v in maps[:3]]        # the width of NaN-free slices
            dev3 = [torch.from_numpy(v).cuda() for v in clean]
            lo_w, hi_w = ic.scale_maps(*clean, scale)
            lo, hi, width = _scale(dev3, scale)
            assert lo.shape == (B, n) and width.shape == (B,) and width.dtype == torch.float32
            assert np.array_equal(_bits(lo.cpu().numpy()), _bits(lo_w)) and np.array_equal(_bits(hi.cpu().numpy()), _bits(hi_w)), (B, n)
            d = hi_w.astype(np.float64) - lo_w.astype(np.float64)
            err = np.abs(width.cpu().numpy().astype(np.float64) - d.mean(1))
            bound = n * 2.0 ** -24 * np.abs(d).max(1)
            print(f"fd_interval_scale_f32 scale={scale} B={B} n={n}: width error / bound {float((err / np.maximum(bound, 1e-300)).max()):.4f}")
            assert (err <= bound).all(), (B, n, err, bound)
            lo_s, hi_s, width_s = _scale(dev3, scale, offset=True)
            assert _same_bits(lo_s, lo) and _same_bits(hi_s, hi) and _same_bits(width_s, width), (B, n)
            for b in range(B):
                one = _scale([t[b:b + 1].clone() for t in dev3], scale)
                assert _same_bits(one[0], lo[b:b + 1]) and _same_bits(one[1], hi[b:b + 1]) and _same_bits(one[2], width[b:b + 1]), (n, b)
            # with the NaNs: they mark their own pixels only, in both forms
            lo_w, hi_w = ic.scale_maps(*maps[:3], scale)
            assert (np.isnan(lo_w).any() or n < 1024) and np.array_equal(np.isnan(lo_w), np.isnan(hi_w))
            for offset in (False, True):
                lo, hi, width = _scale(dev[:3], scale, offset)
                assert np.array_equal(_bits(lo.cpu().numpy()), _bits(lo_w)) and np.array_equal(_bits(hi.cpu().numpy()), _bits(hi_w))
                assert np.array_equal(np.isnan(width.cpu().numpy()), np.isnan(lo_w).any(1))


@pytest.mark.parametrize("n", [7, 4096])
def test_scale_of_maps_inside_a_quantile_tensor(n):
    maps, dev = _case(3, n, 33)
    q = torch.zeros(3, 3, n, device="cuda")
    q[:, 0], q[:, 2] = dev[1], dev[2]
    lo, hi, width = _scale([dev[0], q[:, 0], q[:, 2]], 1.53125)
    ref = _scale(dev[:3], 1.53125)
    assert _same_bits(lo, ref[0]) and _same_bits(hi, ref[1]) and _same_bits(width, ref[2])


# ---- the two kernels against each other
def test_scaled_interval_holds_the_pixels_the_histogram_counts():
    """At scale = grid[g] a pixel is inside [lo_out, hi_out] iff its score is <= scale, except where the float64
    |(m - y) - scale d| on the side concerned is within 8 2^-24 max(|m|, |y|, scale d): the four roundings involved."""
    from founddiff_amd.metrics import interval_hist, interval_scale
    rng = np.random.default_rng(7)
    B, n = 4, 64 * 64
    f = np.float32
    m = rng.uniform(0.4, 0.6, (B, n)).astype(f)
    l = (m - rng.uniform(0, 0.05, (B, n)).astype(f)).astype(f)
    u = (m + rng.uniform(0, 0.05, (B, n)).astype(f)).astype(f)
    for scale in (0.5, 1.0, 2.0, 4.0):
        y = (m + rng.uniform(-0.25, 0.25, (B, n)).astype(f)).astype(f)
        d_lo, d_hi = ic.half_widths(m, l, u)
        y[:, 0::7] = (m - f(scale) * d_lo).astype(f)[:, 0::7]            # planted on both boundaries
        y[:, 3::7] = (m + f(scale) * d_hi).astype(f)[:, 3::7]
        assert y.min() > 0.1 and y.max() < 0.9
        dev = [torch.from_numpy(v).cuda() for v in (m, l, u, y)]
        lo_out, hi_out, _ = interval_scale(*dev[:3], scale)
        assert float(lo_out.min()) > 0 and float(hi_out.max()) < 1        # nothing was clamped
        inside = ((lo_out <= dev[3]) & (dev[3] <= hi_out)).cpu().numpy()
        s, out = ic.score(m, l, u, y)
        counted = ~out & (s <= f(scale))
        h = interval_hist(*dev, [scale]).cpu().numpy()
        assert np.array_equal(h[:, 0], counted.sum(1)) and np.array_equal(h[:, 1], n - counted.sum(1))
        differ = inside != counted
        m64, y64 = m.astype(np.float64), y.astype(np.float64)
        below = y64 < m64
        d = np.where(below, d_lo, d_hi).astype(np.float64)
        gap = np.abs(np.abs(m64 - y64) - scale * d)
        slack = 8 * 2.0 ** -24 * np.maximum(np.maximum(np.abs(m64), np.abs(y64)), scale * d)
        print(f"scale {scale}: {int(differ.sum())} of {B * n} pixels differ, {int((gap <= slack).sum())} within the slack")
        assert (gap[differ] <= slack[differ]).all()
        assert 0.05 < counted.mean() < 0.95


# ---- end to end
N_CAL, K, ALPHA, LEVELS = 12, 4, 0.2, (0.05, 0.95)
# 0, then 2^-4 .. 2^12 in quarter octaves.  With every map in [0, 1] and the floor 1 / 3000 no finite score exceeds 3000, so this
# grid accepts whatever the tiny model with synthetic weights predicts; the default grid ends at 16.
GRID = np.concatenate([[0.0], 2.0 ** (np.arange(-16, 49) / 4)]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _model():
    from _dist_worker import build
    return build("cuda")


def _trainer(folder, n=N_CAL):
    from types import SimpleNamespace
    from founddiff_amd.DADiff import Trainer
    from founddiff_amd.data import SyntheticCTDataset
    ds = SyntheticCTDataset(n, 64)
    tr = Trainer(SimpleNamespace(is_train=False), _model(), None, num_samples=1, condition=True, num_unet=1,
                 checkpoint_folder=str(folder), is_train=False, dataset=ds, val_dataset=ds)
    return tr, ds


@functools.lru_cache(maxsize=None)
def _calibrated(tmp):
    """(trainer, dataset, calibration at batch_size 4): made once for the tests that read it"""
    tr, ds = _trainer(tmp)
    return tr, ds, tr.calibrate_intervals(n_samples=K, quantiles=LEVELS, alpha=ALPHA, grid=GRID, ensemble_seed=40, batch_size=4)


@pytest.fixture(scope="module")
def calibrated(tmp_path_factory):
    return _calibrated(str(tmp_path_factory.mktemp("interval") / "ck"))


def _oracle_counts(ds, levels, centre, grid, **kw):
    x = torch.stack([ds[i][1] for i in range(len(ds))]).cuda()
    y = torch.stack([ds[i][0] for i in range(len(ds))]).numpy().reshape(len(ds), -1)
    ens = _model().sample_ensemble([x], K, slice_seeds=[40 + i for i in range(len(ds))], quantiles=levels, return_samples=True, **kw)
    flat = lambda t: t.cpu().numpy().reshape(len(ds), -1)
    c = flat(ens.mean) if centre is None else flat(ens.quantiles[:, centre])
    return ic.hist(c, flat(ens.quantiles[:, 0]), flat(ens.quantiles[:, 1]), y, grid), ens


def test_calibrate_intervals_is_the_oracles_scale(calibrated):
    from founddiff_amd.ensemble import IntervalCalibration
    tr, ds, cal = calibrated
    grid = GRID
    counts, _ = _oracle_counts(ds, LEVELS, None, grid)
    assert np.array_equal(tr.interval_counts, counts)
    g, scale, R = ic.risk_control(counts, 4096, grid, ALPHA)
    assert isinstance(cal, IntervalCalibration) and tr.interval_calibration is cal
    assert (cal.g, cal.scale, cal.risk) == (g, scale, R.numerator / R.denominator)
    assert (cal.n_slices, cal.n_pixels, cal.alpha, cal.bound, cal.grid_max) == (N_CAL, 4096, ALPHA, "crc", 4096.0)
    assert cal.settings["n_samples"] == K and cal.settings["levels"] == list(LEVELS) and cal.settings["sampler"] == "ddim"
    assert cal.settings["estimate"] == "mean" and cal.settings["floor"] == 1 / 3000 and cal.settings["objective"] == "pred_res"
    # one slice per call: the same counts, the same scale; and the file round-trips
    tr1, _ = _trainer(os.path.join(tr.checkpoint_folder, "one"))
    cal1 = tr1.calibrate_intervals(ds, n_samples=K, quantiles=LEVELS, alpha=ALPHA, grid=GRID, ensemble_seed=40, batch_size=1)
    assert cal1 == cal and np.array_equal(tr1.interval_counts, counts)
    assert os.path.exists(os.path.join(tr1.results_folder, "interval_calibration.json"))
    tr1.interval_calibration = None
    assert tr1.load_interval_calibration() == cal and tr1.interval_calibration == cal
    assert tr1.load_interval_calibration(os.path.join(tr.results_folder, "interval_calibration.json")) == cal
    # the first `items` slices only
    cal6 = tr1.calibrate_intervals(ds, n_samples=K, quantiles=LEVELS, alpha=ALPHA, grid=GRID, ensemble_seed=40, batch_size=4, items=6)
    assert cal6.n_slices == 6 and np.array_equal(tr1.interval_counts, counts[:6])


def test_trainer_test_with_the_calibrated_scale(calibrated):
    from founddiff_amd.metrics import interval_scale
    tr, ds, cal = calibrated
    kw = dict(n_samples=K, ensemble_seed=40, quantiles=LEVELS, batch_size=4)
    tr.test(**kw)
    plain = (list(tr.test_running_psnr), list(tr.test_running_coverage))
    base = [os.path.join(tr.results_folder, ds.load_name(i)[:-4]) for i in range(N_CAL)]
    plain_q = [[np.load(b + s + ".npy") for s in ("", "_std", "_q0050", "_q0950")] for b in base]
    assert not hasattr(tr, "test_running_coverage_calibrated") and not os.path.exists(base[0] + "_lo.npy")
    tr.test(interval_scale="calibrated", **kw)
    assert (list(tr.test_running_psnr), list(tr.test_running_coverage)) == plain
    for b, files in zip(base, plain_q):
        for s, want in zip(("", "_std", "_q0050", "_q0950"), files):
            assert np.array_equal(_bits(np.load(b + s + ".npy")), _bits(want)), (b, s)
    # the same integers as the calibration's
    cov = tr.test_running_coverage_calibrated
    assert len(cov) == N_CAL and len(tr.test_running_interval_width) == N_CAL
    covered = [round(c * 4096) for c in cov]
    assert [c / 4096 for c in covered] == cov
    assert covered == tr.interval_counts[:, :cal.g + 1].sum(1).tolist()
    assert Fraction(sum(covered), N_CAL * 4096) == 1 - Fraction(N_CAL * 4096 - sum(covered), N_CAL * 4096)
    assert cal.risk == (N_CAL * 4096 - sum(covered)) / (N_CAL * 4096) and 1 - cal.risk >= 1 - ALPHA
    assert abs(float(np.mean(cov)) - (1 - cal.risk)) <= 2.0 ** -52
    # the saved maps are interval_scale of the ensemble's maps
    _, ens = _oracle_counts(ds, LEVELS, None, [1.0])
    lo, hi, width = interval_scale(ens.mean, ens.quantiles[:, 0], ens.quantiles[:, 1], cal.scale)
    for i, b in enumerate(base):
        assert np.array_equal(_bits(np.load(b + "_lo.npy")), _bits(lo[i, 0].cpu().numpy())), i
        assert np.array_equal(_bits(np.load(b + "_hi.npy")), _bits(hi[i, 0].cpu().numpy())), i
    assert tr.test_running_interval_width == [float(w) for w in width.cpu().numpy()]
    # a number needs no calibration; another ensemble is refused, and so is a trainer without a calibration
    tr2, ds2 = _trainer(os.path.join(tr.checkpoint_folder, "two"), n=2)
    tr2.test(interval_scale=2.0, n_samples=K, ensemble_seed=40, quantiles=LEVELS)
    _, ens2 = _oracle_counts(ds2, LEVELS, None, [1.0])
    lo2, hi2, width2 = interval_scale(ens2.mean, ens2.quantiles[:, 0], ens2.quantiles[:, 1], 2.0)
    assert tr2.test_running_interval_width == [float(w) for w in width2.cpu().numpy()]
    assert np.array_equal(np.load(os.path.join(tr2.results_folder, ds2.load_name(1)[:-4] + "_hi.npy")), hi2[1, 0].cpu().numpy())
    with pytest.raises(RuntimeError, match="needs a calibration"):
        tr2.test(interval_scale="calibrated", n_samples=K, quantiles=LEVELS)
    with pytest.raises(RuntimeError, match="not valid for this call: n_samples was 4 .* is 3 now"):
        tr.test(interval_scale="calibrated", n_samples=3, ensemble_seed=40, quantiles=LEVELS)
    with pytest.raises(RuntimeError, match="not valid for this call: levels"):
        tr.test(interval_scale="calibrated", n_samples=K, quantiles=(0.1, 0.9))


def test_median_centre_and_flips(tmp_path):
    from founddiff_amd.metrics import interval_scale
    tr, ds = _trainer(tmp_path / "ck")
    grid = GRID
    # around the 0.5 level, which joins the caller's two
    cal = tr.calibrate_intervals(n_samples=K, quantiles=LEVELS, estimate="median", alpha=ALPHA, grid=GRID, ensemble_seed=40, batch_size=4)
    counts, ens = _oracle_counts(ds, LEVELS + (0.5,), 2, grid)
    assert np.array_equal(tr.interval_counts, counts) and cal.settings["estimate"] == "median"
    assert (cal.g, cal.scale) == ic.risk_control(counts, 4096, grid, ALPHA)[:2]
    tr.test(interval_scale="calibrated", n_samples=K, ensemble_seed=40, quantiles=LEVELS, estimate="median", batch_size=4)
    assert [round(c * 4096) for c in tr.test_running_coverage_calibrated] == counts[:, :cal.g + 1].sum(1).tolist()
    lo = interval_scale(ens.quantiles[:, 2], ens.quantiles[:, 0], ens.quantiles[:, 1], cal.scale)[0]
    assert np.array_equal(_bits(np.load(os.path.join(tr.results_folder, ds.load_name(3)[:-4] + "_lo.npy"))), _bits(lo[3, 0].cpu().numpy()))
    with pytest.raises(RuntimeError, match="not valid for this call: estimate"):
        tr.test(interval_scale="calibrated", n_samples=K, ensemble_seed=40, quantiles=LEVELS)
    # an orientation ensemble through both calls
    cal = tr.calibrate_intervals(n_samples=K, quantiles=LEVELS, alpha=ALPHA, grid=GRID, ensemble_seed=40, batch_size=4, orientations="flips")
    counts, _ = _oracle_counts(ds, LEVELS, None, grid, orientations="flips")
    assert np.array_equal(tr.interval_counts, counts) and cal.settings["orientations"] == [0, 1, 2, 3]
    assert (cal.g, cal.scale) == ic.risk_control(counts, 4096, grid, ALPHA)[:2]
    tr.test(interval_scale="calibrated", n_samples=K, ensemble_seed=40, quantiles=LEVELS, batch_size=4, orientations="flips")
    assert [round(c * 4096) for c in tr.test_running_coverage_calibrated] == counts[:, :cal.g + 1].sum(1).tolist()
    with pytest.raises(RuntimeError, match="not valid for this call: orientations"):
        tr.test(interval_scale="calibrated", n_samples=K, ensemble_seed=40, quantiles=LEVELS)
