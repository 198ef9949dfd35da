"""The device-resident slice store and its flip / rot90 augmentation (founddiff_amd.data.DeviceSliceStore,
founddiff_amd.diffusion_train.train_augment / StoreBatch, csrc/fd_train_data.hip), host side, without a GPU: the augmentation code as
a pure function, its distribution, the closed form of the source pixel against numpy, the error paths that need no GPU, the C ABI
of both builds and the scratch of the new kernels."""
import os
import re
import shutil

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("fd_store_gather_f32", "fd_res_qsample_store_f32")


def numpy_augment(m, code):
    """the reference's composition on a (1, H, W) slice: RandomFlip over axes 1 and 2 (its flip over the axis of length 1 is the
    identity), then RandomRotate90 over (1, 2)"""
    if code & 1:
        m = np.flip(m, 1)
    if code & 2:
        m = np.flip(m, 2)
    return np.rot90(m, (code >> 2) & 3, (1, 2))


def test_train_augment_is_a_pure_function_keyed_per_item():
    from founddiff_amd.diffusion_train import _mix64, train_augment
    a = train_augment(5, 3, 1, [7, 2, 9, 7])
    assert a.dtype == np.int32 and a.shape == (4,) and ((a >= 0) & (a < 16)).all()
    assert (a == train_augment(5, 3, 1, [7, 2, 9, 7])).all()
    assert a[0] == a[3]                                                  # the same item twice in one batch
    b = train_augment(5, 3, 1, [1, 7, 4])                                # ... and in another batch
    assert b[1] == a[0]
    assert [int(c) for c in a] == [_mix64(5, 3, 1, i, 0x61) & 15 for i in (7, 2, 9, 7)]
    items = list(range(64))
    base = train_augment(5, 3, 1, items)
    for other in (train_augment(6, 3, 1, items), train_augment(5, 4, 1, items), train_augment(5, 3, 0, items)):
        assert (other != base).any()                                     # seed, step and micro-batch all key it
    ns = train_augment(5, 3, 1, items, square=False)
    assert ((ns >> 2) & 1 == 0).all()                                    # never an odd k on a non-square store
    assert (ns == (base & ~4)).all() and (base & 4).any()
    assert train_augment(5, 3, 1, []).shape == (0,)


def test_train_augment_is_uniform():
    """16 000 items at one (seed, step, micro): expectation 1000 per code, sigma ~ 31; the function is deterministic, so this
    checks the chosen seed"""
    from founddiff_amd.diffusion_train import train_augment
    counts = np.bincount(train_augment(0, 0, 0, range(16000)), minlength=16)
    print(f"[measured] codes of 16 000 items: min {counts.min()} max {counts.max()}")
    assert counts.sum() == 16000 and len(counts) == 16
    assert (counts >= 800).all() and (counts <= 1200).all(), counts
    # the 16 codes reach the 8 elements of the dihedral group twice each
    m = np.arange(36, dtype=np.float32).reshape(1, 6, 6)
    images = [numpy_augment(m, c).tobytes() for c in range(16)]
    assert len(set(images)) == 8 and all(images.count(i) == 2 for i in set(images))


@pytest.mark.parametrize("H,W", [(6, 6), (4, 8)])
def test_source_index_closed_form(H, W):
    """the source pixel (i, j) of output pixel (y, x), as the kernels compute it, against np.rot90(np.flip(...)): all 16 codes on
    a square array, the 8 even-k codes on a non-square one"""
    from founddiff_amd.diffusion_train import augment_source_index
    m = np.random.default_rng(1).random((1, H, W)).astype(np.float32)
    codes = [c for c in range(16) if H == W or not c & 4]
    assert len(codes) == (16 if H == W else 8)
    for code in codes:
        i, j = augment_source_index(code, H, W)
        want = numpy_augment(m, code)
        assert want.shape == (1, H, W) and i.shape == (H, W)
        assert np.array_equal(m[0][i, j], want[0]), code
    if H != W:
        with pytest.raises(RuntimeError, match="transposes"):
            augment_source_index(4, H, W)


def _raises(match, fn, *args, **kw):
    with pytest.raises(RuntimeError, match=match):
        fn(*args, **kw)


def _fake_store(n, H, W):
    """a store that was never constructed (there is no CPU store): what the checks of a batch read"""
    from founddiff_amd.data import DeviceSliceStore
    st = object.__new__(DeviceSliceStore)
    st.n_nd = st.n_ld = n
    st.H, st.W, st.nd_index, st.device = H, W, np.arange(n), torch.device("cpu")
    return st


def test_store_rejects_before_cuda_is_initialised(tmp_path):
    """types, then shapes, then devices; the ranges of indices and codes: each with its message, and nothing touches the GPU"""
    from founddiff_amd import data, diffusion_train as dt
    from founddiff_amd.DADiff import residual_schedule
    S = data.DeviceSliceStore
    was = torch.cuda.is_initialized()
    item = lambda h=4, w=4: [torch.rand(1, h, w), torch.rand(1, h, w)]
    # constructors
    _raises("GPU", S.from_items, [item(), item()], "cpu")
    _raises("mixed slice shapes", S.from_items, [item(), item(4, 6)], "cuda")
    _raises("mixed slice shapes", S.from_items, [[torch.rand(1, 4, 4), torch.rand(1, 4, 6)]], "cuda")
    _raises("empty", S.from_items, [], "cuda")
    _raises("list of", S.from_items, torch.rand(2, 2, 4, 4), "cuda")
    _raises(r"\[ndct, ldct\]", S.from_items, [torch.rand(1, 4, 4)], "cuda")
    _raises("must be a tensor", S.from_items, [[torch.rand(1, 4, 4), "x"]], "cuda")
    _raises("unsupported shape", S.from_items, [[torch.rand(2, 4, 4), torch.rand(2, 4, 4)]], "cuda")
    _raises("__len__", S.from_dataset, 5, "cuda")
    _raises("empty", S.from_dataset, data.CTSliceDataset([], []), "cuda")
    _raises("GPU", S.from_dataset, data.SyntheticCTDataset(2, 8), "cpu")
    _raises("MixedDoseTestDataset", S.from_mixed_dose, data.SyntheticCTDataset(2, 8), "cuda")
    _raises("empty", S.from_mixed_dose, data.MixedDoseTestDataset([], {}), "cuda")
    nd, ld = torch.rand(2, 4, 6), torch.rand(3, 4, 6)
    _raises("must be a tensor", S, nd.numpy(), ld, [0, 1, 1])
    _raises("float32", S, nd.double(), ld, [0, 1, 1])
    _raises("integers", S, nd, ld, [0.0, 1.0, 1.0])
    _raises("inconsistent shapes", S, nd, ld, [0, 1])
    _raises("inconsistent shapes", S, nd, ld[:, :, :4], [0, 1, 1])
    _raises("inconsistent shapes", S, nd, ld, [0, 1, 1], ["a"])
    _raises("empty", S, nd[:0], ld, [0, 0, 0])
    _raises("outside nd", S, nd, ld, [0, 1, 2])
    _raises("GPU", S, nd, ld, [0, 1, 1])
    # a batch: types, shapes, ranges
    sq, ns = _fake_store(5, 8, 8), _fake_store(5, 4, 8)
    for make in (dt.StoreBatch, lambda *a: sq.batch(*a[1:]) if a[0] is sq else ns.batch(*a[1:])):
        _raises("sequence of integers", make, sq, [0.5, 1.0])
        _raises("sequence of integers", make, sq, [0, 1], [0.0, 1.0])
        _raises("inconsistent shapes", make, sq, [])
        _raises("inconsistent shapes", make, sq, [[0, 1]])
        _raises("inconsistent shapes", make, sq, [0, 1], [3])
        _raises(r"index 5 outside \[0, 5\)", make, sq, [0, 5])
        _raises(r"index -1 outside", make, sq, [-1, 2])
        _raises(r"code 16 outside \[0, 16\)", make, sq, [0, 1], [3, 16])
        _raises(r"code -1 outside", make, sq, [0, 1], [-1, 2])
        _raises("transposes", make, ns, [0, 1], [3, 4])
        _raises("transposes", make, ns, [0, 1], [12, 0])
    _raises("DeviceSliceStore", dt.StoreBatch, [nd, ld], [0])
    sb = dt.StoreBatch(ns, [4, 0, 4], [11, 0, 2])                        # even k on a non-square store; a repeated index
    assert len(sb) == 3 and sb.shape == (3, 1, 4, 8) and sb.indices.dtype == np.int64 and sb.codes.tolist() == [11, 0, 2]
    assert dt.StoreBatch(sq, torch.tensor([1, 2])).codes is None
    # q_sample / p_losses_fn / train_step on a StoreBatch
    sch = residual_schedule(1000)
    sb = dt.StoreBatch(sq, [1, 2], [5, 0])
    t, nz = np.array([3, 999]), torch.randn(2, 1, 8, 8)
    fn = lambda x, times: [x[:, :1]]
    _raises("x_input must be None", dt.q_sample, sb, nz, t, sch)
    _raises("must be a tensor or a sequence", dt.q_sample, sb, None, 5, sch)
    _raises("int64", dt.q_sample, sb, None, [0.5, 1.5], sch)
    _raises("int64", dt.q_sample, sb, None, t, sch, None, torch.tensor([1.0, 2.0]))
    _raises("float32", dt.q_sample, sb, None, t, sch, nz.double())
    _raises("either noise or slice_seeds", dt.q_sample, sb, None, t, sch, nz, [1, 2])
    _raises("schedule must be a dict", dt.q_sample, sb, None, t, None)
    _raises("inconsistent shapes", dt.q_sample, sb, None, t[:1], sch)
    _raises("inconsistent shapes", dt.q_sample, sb, None, t, sch, nz[:, :, :4])
    _raises("inconsistent shapes", dt.q_sample, sb, None, t, sch, None, [1, 2, 3])
    _raises("inconsistent shapes", dt.p_losses_fn, fn, sb, t, sch, "pred_res", "l1", nz[:1])
    _raises("unknown objective", dt.p_losses_fn, fn, sb, t, sch, "pred_v")
    opt = object.__new__(dt.ClipAdamEMA)
    _raises("inconsistent shapes", dt.train_step, fn, opt, sb, t[:1], None, [1, 2], 0, sch)
    _raises("lists of 2", dt.train_step, fn, opt, [sb, sb], t, None, None, 0, sch)
    _raises("inconsistent shapes", dt.train_step, fn, opt, [sb, sb], [t[:1], t], None, [[1, 2], [3, 4]], 0, sch)
    assert torch.cuda.is_initialized() == was


def test_trainer_takes_augment():
    """the new keyword defaults to off and leaves augment_flip ignored"""
    import inspect
    from founddiff_amd.DADiff import Trainer
    sig = inspect.signature(Trainer.__init__).parameters
    assert sig["augment"].default is False and sig["augment"].kind is inspect.Parameter.KEYWORD_ONLY
    assert sig["augment_flip"].default is True


def test_new_entries_are_declared_and_exported():
    """declared in include/founddiff_hip.h, present in _lib's table, exported by both builds of the library"""
    from founddiff_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "founddiff_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint " + name + r"\(", hdr), name
        assert name in L.SIGNATURES, name
    assert len(L.SIGNATURES["fd_store_gather_f32"][1]) == 13 and len(L.SIGNATURES["fd_res_qsample_store_f32"][1]) == 24
    for build in (L.BF16, L.F16):
        lib = build.lib()
        for name in NEW_SYMBOLS:
            assert hasattr(lib, name), name


def test_entries_reject_bad_arguments_without_launching():
    """null pointers and shapes outside the limits fail in the entry itself, with a message, before any launch"""
    from founddiff_amd import _lib as L
    one = 16                                                             # never dereferenced: every call fails its checks first
    for build in (L.BF16, L.F16):
        lib = build.lib()
        assert lib.fd_store_gather_f32(None, one, 1, 1, one, one, None, one, one, 1, 4, 4, None) != 0
        assert b"null pointer" in lib.fd_last_error()
        for B, H, W in ((0, 4, 4), (65536, 4, 4), (1, 0, 4), (1, 4, 32769)):
            assert lib.fd_store_gather_f32(one, one, 1, 1, one, one, None, one, one, B, H, W, None) != 0
            assert b"unsupported shape" in lib.fd_last_error()
        assert lib.fd_store_gather_f32(one, one, 0, 1, one, one, None, one, one, 1, 4, 4, None) != 0
        args = [one, one, 1, 1, one, one, None, one, one, one, 1000]
        assert lib.fd_res_qsample_store_f32(*args, one, one, 0, 1, one, one, one, one, None, 1, 4, 4, None) != 0
        assert b"either noise or seeds" in lib.fd_last_error()
        assert lib.fd_res_qsample_store_f32(*args, None, one, 0, 1, one, one, None, one, None, 1, 4, 4, None) != 0
        assert b"noise_out" in lib.fd_last_error()
        assert lib.fd_res_qsample_store_f32(*args[:-1], 0, one, None, 0, 1, one, one, None, one, None, 1, 4, 4, None) != 0
        assert b"unsupported shape" in lib.fd_last_error()


def test_new_kernels_use_no_scratch():
    """0 bytes of scratch per lane for the six instantiations of csrc/fd_train_data.hip's kernel (16-byte / per pixel x gather /
    given noise / keyed noise), in both builds; the 16-byte ones hold the two 64 x 65 tiles in the LDS"""
    if not shutil.which("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    from founddiff_amd import build
    for half in ("bf16", "fp16"):
        build.build(half=half)
        tab = build.resources(half).get("fd_train_data.hip")
        assert tab, "no resource remarks beside fd_train_data.hip's object: rebuild with build(force=True)"
        kernels = {name: r for name, r in tab.items() if "store_batch_kernel" in name}
        assert len(kernels) == 6 and len(tab) == 6, sorted(tab)
        for name, r in kernels.items():
            assert r.get("scratch", 0) == 0, (half, name, r)
            assert r.get("lds", 0) == (2 * 64 * 65 * 4 if "ILb1E" in name else 0), (half, name, r)
