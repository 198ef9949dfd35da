"""Ensemble quantiles on the GPU: fd_ensemble_order_f32 at the C ABI against a stable CPU sort -- exact selections bit for bit,
interpolated levels within the two roundings of fmaf(frac, v_hi - v_lo, v_lo), the sorting networks against the counting path, the
16-byte form against the scalar form, a slice independent of its batch, NaN pixels -- fd_ensemble_coverage_f32 against the CPU count,
and sample_ensemble(quantiles=...) with its callers Trainer.test and sample_volume.  64 x 64, 2 DDIM steps, the tiny model of the
other end-to-end tests."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ORDER, COVERAGE = "fd_ensemble_order_f32", "fd_ensemble_coverage_f32"
LEVELS = (0, 0.05, 0.25, 0.5, 0.75, 0.95, 1)
KS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33)        # every padded size of the networks at and just past its edge, and the counting path
NS = (4, 7, 1024 + 7, 4096)                       # one vector; less than two; two workgroups, the second partly filled; four, full
GENERIC_PAD = 33                                  # K + 33 > 32: the counting path


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _offset_view(t):
    """t's values in memory that starts one float past a 16-byte boundary: the kernels take their scalar path"""
    buf = torch.empty(t.numel() + 4, device=t.device, dtype=t.dtype)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _table(levels, K):
    from founddiff_amd.ensemble import quantile_table
    return quantile_table(levels, K)


def _order(x, table, offset=False):
    """fd_ensemble_order_f32 on x (B, K, n) with the table (lo, hi, frac) -> (B, Q, n); unwritten elements would stay -7"""
    from founddiff_amd import _lib as L
    lo, hi, frac = table
    (B, K, n), Q = x.shape, len(lo)
    x = x.contiguous()
    out = torch.full((B, Q, n), -7.0, device="cuda")
    if offset:
        x, out = _offset_view(x), _offset_view(out)
    else:
        assert x.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    L.call(ORDER, x.data_ptr(), out.data_ptr(), (L.i32 * Q)(*lo.tolist()), (L.i32 * Q)(*hi.tolist()), (L.f32 * Q)(*frac.tolist()),
           B, K, Q, n, _stream())
    return out


@functools.lru_cache(maxsize=None)
def _case(kind, B, K, n):
    """(x on the device, its stable CPU sort over k): computed once, shared by the kernel tests, which leave them unchanged.
    "normal": continuous, both signs; "eighths": multiples of 1/8 in [0, 1], many ties, no -0."""
    g = torch.Generator().manual_seed(1000 * K + 10 * n + B)
    x = torch.randn(B, K, n, generator=g) if kind == "normal" else torch.randint(0, 9, (B, K, n), generator=g).float() / 8
    return x.cuda(), torch.sort(x, dim=1, stable=True).values


def _shapes():
    return [(B, n) for B in (1, 3) for n in NS]


# ---- fd_ensemble_order_f32
@pytest.mark.parametrize("kind", ["normal", "eighths"])
@pytest.mark.parametrize("K", KS)
def test_exact_selections(K, kind):
    """every level whose frac is 0 is the value of that rank in a stable CPU sort, bit for bit"""
    lo, hi, frac = _table(LEVELS, K)
    exact = [j for j in range(len(LEVELS)) if frac[j] == 0]
    assert 0 in exact and len(LEVELS) - 1 in exact                       # minimum and maximum, at every K
    if K in (1, 5, 9, 17, 33):
        assert LEVELS.index(0.5) in exact and LEVELS.index(0.25) in exact and LEVELS.index(0.75) in exact
    if K == 1:
        assert len(exact) == len(LEVELS)
    for B, n in _shapes():
        x, srt = _case(kind, B, K, n)
        for offset in (False, True):
            out = _order(x, (lo, hi, frac), offset).cpu()
            for j in exact:
                assert _same_bits(out[:, j], srt[:, lo[j]]), (B, n, offset, LEVELS[j])


@pytest.mark.parametrize("K", KS)
def test_interpolated_levels(K):
    """|out - ref| <= 3 2^-24 max|v| per pixel, ref the float64 v_lo + frac (v_hi - v_lo) of the CPU sort with the fp32 frac, max|v|
    over the two values: d = v_hi - v_lo rounds once on |d| <= 2 max|v| and is scaled by frac <= 1, the fma rounds once on a
    result of at most max|v|."""
    lo, hi, frac = _table(LEVELS, K)
    worst = 0.0
    for kind in ("normal", "eighths"):
        for B, n in _shapes():
            x, srt = _case(kind, B, K, n)
            s64 = srt.double().numpy()
            out = _order(x, (lo, hi, frac)).cpu().double().numpy()
            for j in range(len(LEVELS)):
                a, b = s64[:, lo[j]], s64[:, hi[j]]
                ref = a + float(frac[j]) * (b - a)
                bound = 3 * 2.0 ** -24 * np.maximum(np.abs(a), np.abs(b))
                err = np.abs(out[:, j] - ref)
                worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
                assert (err <= bound).all(), (kind, B, n, LEVELS[j], worst)
    print(f"fd_ensemble_order_f32 K={K}: worst error / bound {worst:.3f} over {len(LEVELS)} levels")


@pytest.mark.parametrize("K", [k for k in KS if k <= 32])
def test_networks_equal_the_counting_path(K):
    """the K values padded with +inf to K + 33 take the counting path; under the table of K the padding is never selected"""
    tab = _table(LEVELS, K)
    for kind in ("normal", "eighths"):
        for B, n in ((3, 1024 + 7), (1, 4096)):
            x, _ = _case(kind, B, K, n)
            padded = torch.cat([x, torch.full((B, GENERIC_PAD, n), float("inf"), device="cuda")], 1)
            net = _order(x, tab)
            for offset in (False, True):
                assert _same_bits(_order(padded, tab, offset), net), (kind, B, n, offset)
    # and interleaved with the values, so that the counting path's candidates do not arrive in blocks of real ones
    x, _ = _case("eighths", 3, K, 1024 + 7)
    mixed = torch.full((3, 2 * K + GENERIC_PAD, 1024 + 7), float("inf"), device="cuda")
    mixed[:, 1:2 * K:2] = x
    assert _same_bits(_order(mixed, tab), _order(x, tab))


@pytest.mark.parametrize("K", KS)
def test_forms_agree_and_rows_are_independent_of_the_batch(K):
    tab = _table(LEVELS, K)
    for n in NS:
        x, _ = _case("normal", 3, K, n)
        out = _order(x, tab)
        assert not bool((out == -7).any())                               # every element was written
        assert _same_bits(_order(x, tab, offset=True), out), n           # 16-byte (or odd-n scalar) against the offset view
        for b in range(3):
            assert _same_bits(_order(x[b:b + 1].clone(), tab), out[b:b + 1]), (n, b)
    # an odd n is the scalar form of the same pixels: the first 1031 pixels of 4096-pixel slices
    x, _ = _case("normal", 3, K, 4096)
    assert _same_bits(_order(x[:, :, :1031].contiguous(), tab), _order(x, tab)[:, :, :1031])


@pytest.mark.parametrize("K", [1, 5, 8, 32, 33])
def test_a_nan_marks_its_own_pixel_and_no_other(K):
    tab = _table(LEVELS, K)
    for n in (7, 1024 + 7):
        x, _ = _case("normal", 3, K, n)
        ref = _order(x, tab)
        bad = x.clone()
        spots = [(0, 0, 0), (1, K - 1, n - 1), (2, K // 2, n // 2)]
        for b, k, i in spots:
            bad[b, k, i] = float("nan")
        for offset in (False, True):
            out = _order(bad, tab, offset)
            mask = torch.zeros(3, n, dtype=torch.bool, device="cuda")
            for b, k, i in spots:
                mask[b, i] = True
            mask = mask[:, None, :].expand(3, len(LEVELS), n)
            assert bool(torch.isnan(out[mask]).all()) and not bool(torch.isnan(out[~mask]).any())
            assert torch.equal(out[~mask].view(torch.int32), ref[~mask].view(torch.int32))


def test_order_argument_checks():
    from founddiff_amd import _lib as L
    x = torch.zeros(1, 5, 8, device="cuda")
    lo, hi, frac = _table((0.5,), 5)
    with pytest.raises(L.FoundDiffHipError, match="fd_ensemble_order_f32: bad table row"):
        _order(x, (lo, hi + 2, frac))
    nine = np.zeros(9, np.int32)
    with pytest.raises(L.FoundDiffHipError, match="fd_ensemble_order_f32: unsupported shape"):
        _order(x, (nine, nine, np.zeros(9, np.float32)))


# ---- fd_ensemble_coverage_f32
def _cpu_count(lo, hi, t):
    lo, hi, t = (v.cpu().flatten(1) for v in (lo, hi, t))
    return ((t >= lo) & (t <= hi)).sum(1)


@pytest.mark.parametrize("B,n", [(1, 4), (3, 7), (3, 1024 + 7), (2, 4096)])
def test_coverage_counts_exactly(B, n):
    from founddiff_amd.metrics import interval_coverage
    g = torch.Generator().manual_seed(n)
    lo, width, t = (torch.rand(B, n, generator=g).cuda() for _ in range(3))
    hi = lo + 0.5 * width
    count, frac = interval_coverage(lo, hi, t)
    ref = _cpu_count(lo, hi, t)
    assert count.dtype == torch.int64 and count.shape == (B,) and torch.equal(count.cpu(), ref)
    assert frac.dtype == np.float64 and np.array_equal(frac, ref.numpy() / n)
    assert 0 < int(ref.sum()) < B * n or n == 4
    # the scalar form on offset views, and a slice alone
    count_s, _ = interval_coverage(_offset_view(lo), _offset_view(hi), _offset_view(t))
    assert torch.equal(count_s, count)
    for b in range(B):
        assert torch.equal(interval_coverage(lo[b:b + 1], hi[b:b + 1], t[b:b + 1])[0], count[b:b + 1])
    # lo == hi == target: every pixel is inside
    count, frac = interval_coverage(t, t, t)
    assert count.tolist() == [n] * B and frac.tolist() == [1.0] * B
    # a NaN anywhere in a pixel's three values takes that pixel out, and no other
    for which in range(3):
        maps = [t.clone(), t.clone(), t.clone()]
        maps[which][B - 1, n - 1] = float("nan")
        maps[which][0, 0] = float("nan")
        want = [n] * B
        want[0] -= 1
        want[B - 1] -= 1
        assert interval_coverage(*maps)[0].tolist() == want, which


@pytest.mark.parametrize("n", [7, 4096])
def test_coverage_of_maps_inside_a_quantile_tensor(n):
    """lo and hi as rows 1 and 5 of out [B][Q][n]: batch stride Q n, no copy"""
    from founddiff_amd import _lib as L
    from founddiff_amd.metrics import interval_coverage
    x, srt = _case("normal", 3, 9, n)
    out = _order(x, _table(LEVELS, 9))
    t = torch.randn(3, n, generator=torch.Generator().manual_seed(5)).cuda()
    lo, hi = out[:, 1], out[:, 5]
    assert not lo.is_contiguous() and lo.stride(0) == len(LEVELS) * n
    ref = _cpu_count(lo, hi, t)
    assert 0 < int(ref.sum()) < 3 * n
    assert torch.equal(interval_coverage(lo, hi, t)[0].cpu(), ref)
    # the same at the C ABI, on the strides themselves
    nblk = L.lib().fd_ensemble_coverage_nblk(n)
    ws = torch.empty(3 * nblk, device="cuda", dtype=torch.int32)
    count = torch.full((3,), -1, device="cuda", dtype=torch.int64)
    L.call(COVERAGE, lo.data_ptr(), len(LEVELS) * n, hi.data_ptr(), len(LEVELS) * n, t.data_ptr(), n, ws.data_ptr(), count.data_ptr(),
           3, n, _stream())
    assert torch.equal(count.cpu(), ref)


# ---- sample_ensemble(quantiles=...)
SEEDS2 = [11, 2 ** 40 + 5]
STATS = ("mean", "std", "spread")


@functools.lru_cache(maxsize=None)
def _model():
    from _dist_worker import build
    return build("cuda")


@functools.lru_cache(maxsize=None)
def _slices(n):
    from founddiff_amd import synth
    return torch.from_numpy(synth.ct_phantom(n, 64, seed=10)[1]).cuda()


@functools.lru_cache(maxsize=None)
def _ens5():
    """B = 2, K = 5, levels (0, 0.5, 1) with the images, shared by the tests that read it"""
    return _model().sample_ensemble([_slices(2)], 5, slice_seeds=SEEDS2, quantiles=(0, 0.5, 1), return_samples=True)


def test_levels_are_selections_of_the_samples():
    from founddiff_amd.DADiff import EnsembleQuantiles, EnsembleResult
    dif, x = _model(), _slices(2)
    ens = _ens5()
    assert isinstance(ens, EnsembleQuantiles) and ens.levels == (0.0, 0.5, 1.0)
    assert ens.quantiles.shape == (2, 3, 1, 64, 64) and ens.samples.shape == (2, 5, 1, 64, 64)
    srt = torch.sort(ens.samples.cpu(), dim=1, stable=True).values
    assert _same_bits(ens.quantiles[:, 0], ens.samples.amin(1)) and _same_bits(ens.quantiles[:, 2], ens.samples.amax(1))
    assert _same_bits(ens.quantiles[:, 1].cpu(), srt[:, 2])
    assert not torch.equal(ens.quantiles[:, 0], ens.quantiles[:, 2])
    # the call without quantiles: the same statistics and images, the result type of before
    plain = dif.sample_ensemble([x], 5, slice_seeds=SEEDS2, return_samples=True)
    assert isinstance(plain, EnsembleResult) and not hasattr(plain, "quantiles")
    for name in STATS + ("samples",):
        assert _same_bits(getattr(ens, name), getattr(plain, name)), name
    # without return_samples the images stay inside
    quiet = dif.sample_ensemble([x], 5, slice_seeds=SEEDS2, quantiles=(0, 0.5, 1))
    assert quiet.samples is None and _same_bits(quiet.quantiles, ens.quantiles)


def test_k1_levels_are_the_sample():
    dif, x = _model(), _slices(2)
    ens = dif.sample_ensemble([x], 1, slice_seeds=SEEDS2, quantiles=LEVELS)
    assert ens.quantiles.shape == (2, len(LEVELS), 1, 64, 64)
    for j in range(len(LEVELS)):
        assert _same_bits(ens.quantiles[:, j], ens.mean), j


def test_quantiles_independent_of_batch_split_and_streams():
    dif, x = _model(), _slices(2)
    ref = _ens5()
    for b in range(2):
        one = dif.sample_ensemble([x[b:b + 1]], 5, slice_seeds=SEEDS2[b:b + 1], quantiles=(0, 0.5, 1))
        assert _same_bits(one.quantiles, ref.quantiles[b:b + 1]), b
    saved = dif.max_sub_batch, dif.streams
    try:
        dif.max_sub_batch, dif.streams = 2, 2                            # 10 rows: passes of 4 + 4 + 2 against one
        cut = dif.sample_ensemble([x], 5, slice_seeds=SEEDS2, quantiles=(0, 0.5, 1))
        dif.max_sub_batch, dif.streams = saved[0], 1
        one = dif.sample_ensemble([x], 5, slice_seeds=SEEDS2, quantiles=(0, 0.5, 1))
    finally:
        dif.max_sub_batch, dif.streams = saved
    assert _same_bits(cut.quantiles, ref.quantiles) and _same_bits(one.quantiles, ref.quantiles)


@pytest.mark.parametrize("fuse", ["final", "step"])
def test_tiled_quantiles(fuse):
    from founddiff_amd.metrics import ensemble_quantiles
    dif, x = _model(), _slices(2)
    levels = (0.05, 0.5, 0.95)
    kw = dict(slice_seeds=SEEDS2, tile=32, overlap=8, tile_fuse=fuse)
    ens = dif.sample_ensemble([x], 3, quantiles=levels, return_samples=True, **kw)
    assert ens.quantiles.shape == (2, 3, 1, 64, 64) and ens.levels == levels
    assert _same_bits(ens.quantiles, ensemble_quantiles(ens.samples, levels))
    assert _same_bits(ens.quantiles[:, 1].cpu(), torch.sort(ens.samples.cpu(), dim=1, stable=True).values[:, 1])
    plain = dif.sample_ensemble([x], 3, **kw)                            # "final": no images are written here
    assert plain.samples is None
    for name in STATS:
        assert _same_bits(getattr(ens, name), getattr(plain, name)), name
    quiet = dif.sample_ensemble([x], 3, quantiles=levels, **kw)
    assert quiet.samples is None and _same_bits(quiet.quantiles, ens.quantiles)
    for name in STATS:
        assert _same_bits(getattr(quiet, name), getattr(plain, name)), name


# ---- the callers
def _trainer(tmp_path):
    from types import SimpleNamespace
    from founddiff_amd.DADiff import Trainer
    from founddiff_amd.data import SyntheticCTDataset
    ds = SyntheticCTDataset(2, 64)
    tr = Trainer(SimpleNamespace(is_train=False), _model(), None, num_samples=1, condition=True, num_unet=1,
                 checkpoint_folder=str(tmp_path / "ck"), is_train=False, dataset=ds)
    y = torch.stack([ds[i][0] for i in range(2)]).cuda()
    x = torch.stack([ds[i][1] for i in range(2)]).cuda()
    return tr, ds, x, y


def test_trainer_test_saves_the_levels_and_measures_coverage(tmp_path):
    from founddiff_amd.metrics import compute_metrics, interval_coverage
    tr, ds, x, y = _trainer(tmp_path)
    psnr, ssim, rmse = tr.test(n_samples=3, ensemble_seed=40, quantiles=(0.05, 0.95))
    ens = _model().sample_ensemble([x], 3, slice_seeds=[40, 41], quantiles=(0.05, 0.95))
    m = compute_metrics(ens.mean, y).cpu().numpy()                       # the estimate is still the mean
    assert np.array_equal(np.array(tr.test_running_psnr), m[:, 0]) and psnr == float(np.mean(m[:, 0]))
    for i in range(2):
        base = os.path.join(tr.results_folder, ds.load_name(i)[:-4])
        assert np.array_equal(np.load(base + ".npy"), ens.mean[i, 0].cpu().numpy())
        assert np.array_equal(np.load(base + "_std.npy"), ens.std[i, 0].cpu().numpy())
        for j, suffix in enumerate(("_q0050", "_q0950")):
            got = np.load(base + suffix + ".npy")
            assert got.shape == (64, 64) and np.array_equal(got, ens.quantiles[i, j, 0].cpu().numpy()), (i, suffix)
    cover = interval_coverage(ens.quantiles[:, 0], ens.quantiles[:, 1], y)[1]
    assert len(tr.test_running_coverage) == 2 and all(0.0 <= c <= 1.0 for c in tr.test_running_coverage)
    assert tr.test_running_coverage == cover.tolist()
    assert np.array_equal(cover, _cpu_count(ens.quantiles[:, 0], ens.quantiles[:, 1], y).numpy() / 4096)
    # the interval is [lowest level, highest level] whatever the order, one slice per call included
    tr.test(n_samples=3, ensemble_seed=40, quantiles=(0.95, 0.5, 0.05), batch_size=1)
    assert tr.test_running_coverage == cover.tolist()
    assert os.path.exists(os.path.join(tr.results_folder, ds.load_name(0)[:-4] + "_q0500.npy"))


def test_trainer_test_estimate_median(tmp_path):
    from founddiff_amd.metrics import compute_metrics
    tr, ds, x, y = _trainer(tmp_path)
    psnr, ssim, rmse = tr.test(n_samples=3, ensemble_seed=40, estimate="median")
    ens = _model().sample_ensemble([x], 3, slice_seeds=[40, 41], quantiles=(0.5,))
    m = compute_metrics(ens.quantiles[:, 0], y).cpu().numpy()
    assert np.array_equal(np.array(tr.test_running_psnr), m[:, 0]) and np.array_equal(np.array(tr.test_running_ssim), m[:, 1])
    assert np.array_equal(np.array(tr.test_running_rmse), m[:, 2])
    assert (psnr, ssim, rmse) == tuple(float(np.mean(m[:, c])) for c in range(3))
    assert not np.array_equal(m, compute_metrics(ens.mean, y).cpu().numpy())
    assert tr.test_running_coverage == []
    for i in range(2):
        base = os.path.join(tr.results_folder, ds.load_name(i)[:-4])
        assert np.array_equal(np.load(base + ".npy"), ens.quantiles[i, 0, 0].cpu().numpy())
        assert not os.path.exists(base + "_q0500.npy")                   # the internal level is not the caller's
    # with the median among the caller's levels it is saved too, and scored
    psnr2, _, _ = tr.test(n_samples=3, ensemble_seed=40, quantiles=(0.05, 0.5), estimate="median")
    assert psnr2 == psnr
    assert np.array_equal(np.load(os.path.join(tr.results_folder, ds.load_name(1)[:-4] + "_q0500.npy")),
                          ens.quantiles[1, 0, 0].cpu().numpy())


def test_sample_volume_quantiles():
    from founddiff_amd import parallel
    dif, vol = _model(), _slices(3)
    out = parallel.sample_volume(dif, vol, noise_seed=100, batch=2, n_samples=3, quantiles=(0.5,))        # batches of 2 + 1 slices
    assert len(out) == 3
    mean, std, q = out
    ens = dif.sample_ensemble([vol], 3, slice_seeds=[100, 101, 102], quantiles=(0.5,))
    assert q.shape == (3, 1, 1, 64, 64)
    assert _same_bits(mean, ens.mean) and _same_bits(std, ens.std) and _same_bits(q, ens.quantiles)
    assert len(parallel.sample_volume(dif, vol[:1], noise_seed=100, n_samples=3)) == 2                    # without levels: as before


def test_argument_errors(tmp_path):
    from founddiff_amd import parallel
    dif, x = _model(), _slices(2)
    tr = _trainer(tmp_path)[0]
    with pytest.raises(RuntimeError, match="need an ensemble, n_samples > 1"):
        tr.test(quantiles=(0.05, 0.95))
    with pytest.raises(RuntimeError, match="need an ensemble, n_samples > 1"):
        tr.test(n_samples=1, estimate="median")
    with pytest.raises(RuntimeError, match="sample_volume: quantiles need an ensemble"):
        parallel.sample_volume(dif, x, quantiles=(0.5,))
    with pytest.raises(RuntimeError, match="quantile_table: 1 to 8 levels"):
        dif.sample_ensemble([x], 3, quantiles=(0.1,) * 9)
    with pytest.raises(RuntimeError, match="quantile_table: levels must be finite"):
        dif.sample_ensemble([x], 3, quantiles=(0.5, 1.5))
