"""Training on random crops (founddiff_amd.diffusion_train.train_crop / crop_source_index, StoreBatch(..., windows, crop),
Trainer(crop_size=...), csrc/fd_train_crop.hip), host side, without a GPU: the window draw as a pure function, its range and
distribution, the closed form of the source pixel against numpy's slice + reflect pad + flip / rot90, the error paths that need no
GPU, the C ABI of both builds and the resources of the new kernels."""
import inspect
import os
import re
import shutil

import numpy as np
import pytest
import torch

from test_train_data_cpu import _fake_store, _raises, numpy_augment

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("fd_store_crop_f32", "fd_res_qsample_crop_f32")
# (H, W, ch, cw): inside the slice (square and not), the whole slice, padded (even and odd pads), a slice with W % 4 != 0, a pad of
# almost the slice, and the tiled form's 64 + 4 crop
SHAPES = [(20, 28, 8, 8), (20, 28, 8, 12), (20, 28, 20, 28), (20, 28, 24, 32), (20, 28, 23, 31), (13, 11, 8, 8), (6, 6, 11, 11),
          (72, 72, 68, 68)]


def numpy_crop(m, y0, x0, ch, cw):
    """the reference's CropToFixed on a (1, H, W) slice at a given start: a plain slice, then np.pad(mode="reflect") to the crop,
    half of the missing rows / columns (rounded down) in front"""
    c = m[:, y0:y0 + ch, x0:x0 + cw]
    ph, pw = ch - c.shape[1], cw - c.shape[2]
    return np.pad(c, ((0, 0), (ph // 2, ph - ph // 2), (pw // 2, pw - pw // 2)), mode="reflect")


def windows_of(H, W, ch, cw):
    """every x0 % 4 (and the largest x0), y0 at 0, the middle and the maximum"""
    ny, nx = max(H - ch, 1), max(W - cw, 1)
    return [(y0, x0) for y0 in sorted({0, ny // 2, ny - 1}) for x0 in sorted(set(range(min(4, nx))) | {nx - 1})]


def codes_of(ch, cw):
    return [c for c in range(16) if ch == cw or not c & 4]


def test_train_crop_is_a_pure_function_keyed_per_item():
    from founddiff_amd.diffusion_train import _mix64, train_crop
    a = train_crop(5, 3, 1, [7, 2, 9, 7], 20, 28, (8, 12))
    assert a.dtype == np.int64 and a.shape == (4, 2)
    assert np.array_equal(a, train_crop(5, 3, 1, [7, 2, 9, 7], 20, 28, (8, 12)))
    assert (a[0] == a[3]).all()                                          # the same item twice in one batch
    assert (train_crop(5, 3, 1, [1, 7, 4], 20, 28, (8, 12))[1] == a[0]).all()      # ... and in another batch
    assert a.tolist() == [[_mix64(5, 3, 1, i, 0x63) % 12, _mix64(5, 3, 1, i, 0x64) % 16] for i in (7, 2, 9, 7)]
    items = list(range(64))
    base = train_crop(5, 3, 1, items, 20, 28, 8)
    for other in (train_crop(6, 3, 1, items, 20, 28, 8), train_crop(5, 4, 1, items, 20, 28, 8), train_crop(5, 3, 0, items, 20, 28, 8)):
        assert (other[:, 0] != base[:, 0]).any() and (other[:, 1] != base[:, 1]).any()     # seed, step and micro-batch all key it
    assert np.array_equal(train_crop(5, 3, 1, items, 20, 28, (8, 8)), base)                # an int is the square crop
    # the crop is at least the slice: the start is 0, on either axis alone too
    assert not train_crop(5, 3, 1, items, 20, 28, (20, 28)).any() and not train_crop(5, 3, 1, items, 20, 28, (24, 32)).any()
    mixed = train_crop(5, 3, 1, items, 20, 28, (24, 8))
    assert not mixed[:, 0].any() and mixed[:, 1].any()
    assert train_crop(5, 3, 1, [], 20, 28, 8).shape == (0, 2)
    with pytest.raises(RuntimeError, match="crop must be an int"):
        train_crop(5, 3, 1, items, 20, 28, 8.0)


def test_train_crop_range_and_uniformity():
    """16 000 items at (0, 0, 0) with H - ch = W - cw = 8: the range is exactly range(8) -- the reference's randint(max - crop)
    never draws the last possible offset 8 -- and every offset comes 2000 times, sigma ~ 42; the function is deterministic, so this
    checks the chosen keys"""
    from founddiff_amd.diffusion_train import train_crop
    w = train_crop(0, 0, 0, range(16000), 16, 24, (8, 16))
    for axis in (0, 1):
        counts = np.bincount(w[:, axis], minlength=9)
        print(f"[measured] axis {axis}: offsets of 16 000 items: min {counts[:8].min()} max {counts[:8].max()}, offset 8: {counts[8]}")
        assert len(counts) == 9 and counts[8] == 0 and counts.sum() == 16000
        assert set(w[:, axis].tolist()) == set(range(8))
        assert (counts[:8] >= 1800).all() and (counts[:8] <= 2200).all(), counts
    assert (w[:, 0] != w[:, 1]).any()                                    # two keys, not one draw used twice


@pytest.mark.parametrize("H,W,ch,cw", SHAPES)
def test_crop_source_index_closed_form(H, W, ch, cw):
    """the source pixel (i, j) of output pixel (y, x), as the kernels compute it, against numpy: all 16 codes on a square crop, the
    8 even-k codes on a non-square one"""
    from founddiff_amd.diffusion_train import crop_source_index
    m = np.random.default_rng(H * 100 + cw).random((1, H, W)).astype(np.float32)
    codes, wins = codes_of(ch, cw), windows_of(H, W, ch, cw)
    assert len(codes) == (16 if ch == cw else 8)
    assert {x0 % 4 for _, x0 in wins} == set(range(min(4, max(W - cw, 1))))
    for y0, x0 in wins:
        cropped = numpy_crop(m, y0, x0, ch, cw)
        assert cropped.shape == (1, ch, cw)
        for code in codes:
            i, j = crop_source_index(code, y0, x0, H, W, ch, cw)
            want = numpy_augment(cropped, code)
            assert i.shape == j.shape == (ch, cw) and i.min() >= 0 and i.max() < H and j.min() >= 0 and j.max() < W
            assert np.array_equal(m[0][i, j], want[0]), (y0, x0, code)
    if ch != cw:
        with pytest.raises(RuntimeError, match="transposes"):
            crop_source_index(4, 0, 0, H, W, ch, cw)


def test_crop_rejects_before_cuda_is_initialised(tmp_path):
    """types, then shapes, then ranges, each with its message, and nothing touches the GPU"""
    from founddiff_amd import diffusion_train as dt
    from founddiff_amd.DADiff import ResidualDiffusion, Trainer, UnetRes, residual_schedule
    was = torch.cuda.is_initialized()
    sq, ns = _fake_store(5, 8, 8), _fake_store(5, 20, 28)
    for make in (dt.StoreBatch, lambda st, *a, **kw: st.batch(*a, **kw)):
        # types
        _raises("crop must be an int", make, ns, [0, 1], None, None, 8.0)
        _raises("crop must be an int", make, ns, [0, 1], None, None, (8, 8, 8))
        _raises("crop must be an int", make, ns, [0, 1], None, None, (8, 2.5))
        _raises("crop must be an int", make, ns, [0, 1], None, None, True)
        _raises("sequence of integers", make, ns, [0, 1], None, [[0.5, 1.0], [0.0, 0.0]], 8)
        _raises("windows need a crop", make, ns, [0, 1], None, [[0, 0], [0, 0]])
        # shapes
        _raises("inconsistent shapes", make, ns, [0, 1], None, [[0, 0]], 8)
        _raises("inconsistent shapes", make, ns, [0, 1], None, [0, 0], 8)
        _raises("inconsistent shapes", make, ns, [0, 1], None, [[0, 0, 0], [0, 0, 0]], 8)
        _raises("inconsistent shapes", make, ns, [0, 1], [0], [[0, 0], [0, 0]], 8)
        _raises("unsupported shape", make, ns, [0, 1], None, None, 0)
        _raises("unsupported shape", make, ns, [0, 1], None, None, (8, 32769))
        _raises("unsupported shape", make, sq, [0, 1], None, None, 23)                     # pads 7 + 8 of 8 rows: 8 > H - 1
        _raises("unsupported shape", make, ns, [0, 1], None, None, (8, 83))                # pads 27 + 28 of 28 columns
        # ranges
        _raises(r"window \(12, 0\) outside \[0, 12\) x \[0, 20\)", make, ns, [0, 1], None, [[0, 0], [12, 0]], 8)
        _raises(r"window \(0, 20\) outside", make, ns, [0, 1], None, [[0, 20], [0, 0]], 8)
        _raises(r"window \(-1, 3\) outside", make, ns, [0, 1], None, [[-1, 3], [0, 0]], 8)
        _raises(r"window \(1, 0\) outside \[0, 1\) x \[0, 1\)", make, ns, [0, 1], None, [[0, 0], [1, 0]], (20, 28))
        _raises(r"window \(0, 1\) outside \[0, 1\) x \[0, 1\)", make, ns, [0, 1], None, [[0, 1], [0, 0]], (24, 32))
        _raises(r"index 5 outside", make, ns, [0, 5], None, None, 8)
        _raises(r"code 16 outside", make, ns, [0, 1], [3, 16], None, 8)
        _raises(r"code 4 transposes \(k odd\), the crop is 8 x 12", make, ns, [0, 1], [3, 4], None, (8, 12))
        _raises(r"code 12 transposes \(k odd\), the crop is 20 x 28", make, ns, [0, 1], [12, 0], None, (20, 28))
        # without a crop everything is as before
        _raises("transposes .*the store's slices are 20 x 28", make, ns, [0, 1], [3, 4])
    # accepted: a transposing code with a square crop on a non-square store; the largest legal pad; a repeated index
    sb = dt.StoreBatch(ns, [4, 0, 4], [13, 4, 2], [[11, 19], [0, 3], [5, 0]], 8)
    assert len(sb) == 3 and sb.shape == (3, 1, 8, 8) and sb.crop == (8, 8) and sb.codes.tolist() == [13, 4, 2]
    assert sb.windows.dtype == np.int64 and sb.windows.tolist() == [[11, 19], [0, 3], [5, 0]]
    sb = dt.StoreBatch(sq, [1, 2], [11, 0], None, (22, 12))                                 # pads 7 + 7 of 8 rows
    assert sb.shape == (2, 1, 22, 12) and sb.windows is None and sb.crop == (22, 12)
    assert dt.StoreBatch(sq, [1], None, torch.tensor([[1, 3]]), (4, np.int64(4))).windows.tolist() == [[1, 3]]
    plain = dt.StoreBatch(ns, [0, 1], [3, 2])
    assert plain.shape == (2, 1, 20, 28) and plain.crop is None and plain.windows is None
    # q_sample follows the crop's shape
    sch = residual_schedule(1000)
    sb = dt.StoreBatch(ns, [1, 2], [5, 0], [[3, 1], [0, 0]], 8)
    _raises("inconsistent shapes", dt.q_sample, sb, None, np.array([3, 999]), sch, torch.randn(2, 1, 20, 28))
    _raises("inconsistent shapes", dt.p_losses_fn, lambda x, times: [x[:, :1]], sb, np.array([3, 999]), sch, "pred_res", "l1",
            torch.randn(2, 1, 8, 12))
    # Trainer(crop_size=...): multiples of 2 ** (levels - 1), checked in the constructor
    def model(mults):
        net = UnetRes(64, dim_mults=mults, num_unet=1, condition=True, objective="pred_res",
                      clip_cfg=dict(layers=(1, 1, 1, 1), width=16, embed_dim=1024))
        return ResidualDiffusion(net, image_size=64, objective="pred_res", condition=True)
    two, four = model((1, 2)), model((1, 2, 4, 8))
    kw = dict(checkpoint_folder=str(tmp_path), device="cpu")
    assert Trainer(None, two, crop_size=20, **kw).crop_size == (20, 20)                    # 20 is a multiple of 2 ...
    _raises("multiples of 8", Trainer, None, four, crop_size=20, **kw)                     # ... and not of 8
    assert Trainer(None, four, crop_size=(24, 64), **kw).crop_size == (24, 64)
    _raises("multiples of 2", Trainer, None, two, crop_size=(20, 21), **kw)
    _raises("multiples of 2", Trainer, None, two, crop_size=0, **kw)
    _raises("crop_size must be an int", Trainer, None, two, crop_size=20.0, **kw)
    assert Trainer(None, two, **kw).crop_size is None
    assert torch.cuda.is_initialized() == was


def test_trainer_takes_crop_size():
    """keyword-only, after augment, off by default"""
    from founddiff_amd.DADiff import Trainer
    sig = inspect.signature(Trainer.__init__).parameters
    assert sig["crop_size"].default is None and sig["crop_size"].kind is inspect.Parameter.KEYWORD_ONLY
    names = list(sig)
    assert names.index("crop_size") == names.index("augment") + 1
    assert "crop_size" in Trainer.__doc__


def test_new_entries_are_declared_and_exported():
    """declared in include/founddiff_hip.h, present in _lib's table, exported by both builds of the library"""
    from founddiff_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "founddiff_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint " + name + r"\(", hdr), name
        assert name in L.SIGNATURES, name
    # the existing pair plus windows, CH and CW
    assert len(L.SIGNATURES["fd_store_crop_f32"][1]) == 13 + 3 and len(L.SIGNATURES["fd_res_qsample_crop_f32"][1]) == 24 + 3
    for build in (L.BF16, L.F16):
        lib = build.lib()
        for name in NEW_SYMBOLS:
            assert hasattr(lib, name), name


def test_entries_reject_bad_arguments_without_launching():
    """null pointers, shapes outside the limits and a pad that needs a second reflection fail in the entry itself, with a message,
    before any launch"""
    from founddiff_amd import _lib as L
    one = 16                                                             # never dereferenced: every call fails its checks first
    bad_shapes = ((0, 4, 4, 4, 4), (65536, 4, 4, 4, 4), (1, 0, 4, 4, 4), (1, 4, 32769, 4, 4), (1, 4, 4, 0, 4), (1, 4, 4, 4, 32769),
                  (1, 4, 4, 11, 4), (1, 4, 4, 4, 12))                    # pads 3 + 4 and 4 + 4 of 4: more than H - 1 = 3
    for build in (L.BF16, L.F16):
        lib = build.lib()
        assert lib.fd_store_crop_f32(None, one, 1, 1, one, one, None, None, one, one, 1, 4, 4, 4, 4, None) != 0
        assert b"fd_store_crop_f32: null pointer" in lib.fd_last_error()
        assert lib.fd_store_crop_f32(one, one, 1, 1, one, one, None, None, one, None, 1, 4, 4, 4, 4, None) != 0
        assert b"null pointer" in lib.fd_last_error()
        for B, H, W, CH, CW in bad_shapes:
            assert lib.fd_store_crop_f32(one, one, 1, 1, one, one, None, one, one, one, B, H, W, CH, CW, None) != 0
            assert b"fd_store_crop_f32: unsupported shape" in lib.fd_last_error(), (B, H, W, CH, CW)
        assert lib.fd_store_crop_f32(one, one, 0, 1, one, one, None, None, one, one, 1, 4, 4, 4, 4, None) != 0
        assert b"unsupported shape" in lib.fd_last_error()
        args = [one, one, 1, 1, one, one, None, None, one, one, one, 1000]
        tail = [1, 4, 4, 4, 4, None]
        assert lib.fd_res_qsample_crop_f32(*args, one, one, 0, 1, one, one, one, one, None, *tail) != 0
        assert b"either noise or seeds" in lib.fd_last_error()
        assert lib.fd_res_qsample_crop_f32(*args, None, None, 0, 1, one, one, one, one, None, *tail) != 0
        assert b"either noise or seeds" in lib.fd_last_error()
        assert lib.fd_res_qsample_crop_f32(*args, None, one, 0, 1, one, one, None, one, None, *tail) != 0
        assert b"noise_out" in lib.fd_last_error()
        assert lib.fd_res_qsample_crop_f32(*args, one, None, 0, 1, one, None, None, one, None, *tail) != 0
        assert b"fd_res_qsample_crop_f32: null pointer" in lib.fd_last_error()
        assert lib.fd_res_qsample_crop_f32(*args[:-1], 0, one, None, 0, 1, one, one, None, one, None, *tail) != 0       # T = 0
        assert b"unsupported shape" in lib.fd_last_error()
        for B, H, W, CH, CW in bad_shapes:
            assert lib.fd_res_qsample_crop_f32(*args, one, None, 0, 1, one, one, None, one, None, B, H, W, CH, CW, None) != 0
            assert b"fd_res_qsample_crop_f32: unsupported shape" in lib.fd_last_error(), (B, H, W, CH, CW)


def test_new_kernels_use_no_scratch():
    """0 bytes of scratch per lane for the six instantiations of csrc/fd_train_crop.hip's kernel (16-byte / per pixel x gather /
    given noise / keyed noise), in both builds; the 16-byte ones hold the two 64 x 65 tiles in the LDS, the per-pixel ones nothing"""
    if not shutil.which("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    from founddiff_amd import build
    for half in ("bf16", "fp16"):
        build.build(half=half)
        tab = build.resources(half).get("fd_train_crop.hip")
        assert tab, "no resource remarks beside fd_train_crop.hip's object: rebuild with build(force=True)"
        kernels = {name: r for name, r in tab.items() if "crop_batch_kernel" in name}
        assert len(kernels) == 6 and len(tab) == 6, sorted(tab)
        for name, r in kernels.items():
            assert r.get("scratch", 0) == 0, (half, name, r)
            assert r.get("lds", 0) == (2 * 64 * 65 * 4 if "ILb1E" in name else 0), (half, name, r)
