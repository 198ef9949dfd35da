"""The selective-scan backward's host side, without a GPU: the C ABI of both builds of the library and the Python
binding's argument checks (founddiff_amd/selective_scan_train.py)."""
import ctypes

import pytest
import torch


def test_both_libraries_export_the_backward():
    from founddiff_amd import _lib as L
    for build in (L.BF16, L.F16):
        lib = build.lib()
        assert hasattr(lib, "fd_selective_scan_bwd_f32") and hasattr(lib, "fd_selective_scan_bwd_ws_floats")


def test_workspace_size_at_level0():
    """the level-0 training shape (batch 2, KD = 512, K = 4, N = 4, L = 65536): tile composites and parameter partials,
    and nothing for invalid shapes"""
    from founddiff_amd import _lib as L
    for build in (L.BF16, L.F16):
        lib = build.lib()
        n = lib.fd_selective_scan_bwd_ws_floats(2, 512, 4, 4, 65536)
        assert n > 0 and n % 4 == 0
        assert n >= 3 * 256 * 2 * 512 * 4                  # Pa, h and g carries of every (tile, row, state)
        # exactly: the geometry query's 256 tiles and single row split (2 x 4 x 256 workgroups fill the chip) leave the three
        # composite arrays [tile][batch KD][N] and the parameter partials [N + 2][KD][batch][tile], no dB / dC slabs
        out = (ctypes.c_int32 * 8)()
        assert lib.fd_selective_scan_bwd_geom(2, 512, 4, 4, 65536, out) == 0
        assert list(out) == [256, 64, 256, 1, 4, 128, 128, 0]
        ntiles, S = out[0], out[3]
        assert n == 3 * ntiles * 2 * 512 * 4 + (4 + 2) * 512 * 2 * ntiles + (0 if S == 1 else 2 * S * 2 * 4 * 4 * 65536) == 4718592
        assert lib.fd_selective_scan_bwd_ws_floats(2, 510, 4, 4, 65536) == 0
        assert lib.fd_selective_scan_bwd_ws_floats(0, 512, 4, 4, 65536) == 0


def test_train_bwd_rejects_cpu_tensors():
    from founddiff_amd import selective_scan_train as m
    was = torch.cuda.is_initialized()
    b, KD, K, N, L = 1, 8, 2, 3, 16
    u, delta, dout = torch.randn(b, KD, L), torch.randn(b, KD, L), torch.randn(b, KD, L)
    A, Bm, Cm = -torch.rand(KD, N), torch.randn(b, K, N, L), torch.randn(b, K, N, L)
    with pytest.raises(RuntimeError, match="GPU"):
        m.bwd(u, delta, A, Bm, Cm, None, None, dout, torch.zeros(b, KD, N), True, 1)
    assert torch.cuda.is_initialized() == was


def test_train_module_binds_the_sampling_forward_and_the_sampling_module_stays_forward_only():
    from founddiff_amd import selective_scan_cuda_core as core
    from founddiff_amd import selective_scan_train as m
    assert m.fwd is core.fwd and m.bwd is not core.bwd
    with pytest.raises(NotImplementedError):
        core.bwd()
