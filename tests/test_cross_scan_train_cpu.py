"""The fused cross_selective_scan's host side, without a GPU: the C ABI of both builds of the library and the Python binding's
argument checks (founddiff_amd/cross_scan_train.py)."""
import inspect

import pytest
import torch


def test_both_libraries_export_the_cross_scan():
    from founddiff_amd import _lib as L
    for build in (L.BF16, L.F16):
        lib = build.lib()
        for name in ("fd_cross_scan_fwd_f32", "fd_cross_scan_bwd_f32", "fd_cross_scan_bwd_ws_floats"):
            assert hasattr(lib, name), name


def test_workspace_size_at_level0():
    """down0 of the training shape (batch 2, 512 x 512, d_inner 128, N 4, R 4): tile carries, partials and the dxdbl rows;
    nothing for shapes the kernels do not serve"""
    from founddiff_amd import _lib as L
    for build in (L.BF16, L.F16):
        lib = build.lib()
        n = lib.fd_cross_scan_bwd_ws_floats(2, 512, 512, 128, 4, 4)
        assert n > 0 and n % 4 == 0
        assert n >= 4 * 2 * 256 * 256 * 12                  # the complete dxdbl rows of every direction and position
        assert lib.fd_cross_scan_bwd_ws_floats(2, 512, 512, 96, 4, 4) == 0       # d_inner not a multiple of 64
        assert lib.fd_cross_scan_bwd_ws_floats(2, 512, 512, 128, 6, 4) == 0      # d_state
        assert lib.fd_cross_scan_bwd_ws_floats(2, 512, 512, 128, 4, 3) == 0      # dt_rank
        assert lib.fd_cross_scan_bwd_ws_floats(0, 512, 512, 128, 4, 4) == 0


def test_signature_is_the_references():
    """src/emamba2.py:295-308: cross_selective_scan(x=None, x_proj_weight=None, x_proj_bias=None, dt_projs_weight=None,
    dt_projs_bias=None, A_logs=None, Ds=None, out_norm=None, nrows=-1, delta_softplus=True, to_dtype=True, step_size=2)"""
    from founddiff_amd.cross_scan_train import cross_selective_scan
    ref = [("x", inspect.Parameter.empty), ("x_proj_weight", None), ("x_proj_bias", None), ("dt_projs_weight", None),
           ("dt_projs_bias", None), ("A_logs", None), ("Ds", None), ("out_norm", None), ("nrows", -1),
           ("delta_softplus", True), ("to_dtype", True), ("step_size", 2)]
    got = [(p.name, p.default) for p in inspect.signature(cross_selective_scan).parameters.values()]
    assert [n for n, _ in got] == [n for n, _ in ref]
    # the reference gives x a default of None too; every caller passes it
    assert got[1:] == ref[1:]


def _cpu_args(D=64, N=4, R=4, H=8, W=8):
    return dict(x=torch.randn(1, D, H, W), x_proj_weight=torch.randn(4, R + 2 * N, D), dt_projs_weight=torch.randn(4, D, R),
                dt_projs_bias=torch.randn(4, D), A_logs=torch.randn(4 * D, N), Ds=torch.ones(4 * D))


def test_rejects_before_cuda_is_initialised():
    """CPU tensors, an x_proj bias, step_size 3 and delta_softplus=False raise RuntimeError before anything touches the GPU"""
    from founddiff_amd.cross_scan_train import cross_selective_scan
    was = torch.cuda.is_initialized()
    a = _cpu_args()
    with pytest.raises(RuntimeError, match="GPU"):
        cross_selective_scan(**a)
    with pytest.raises(RuntimeError, match="x_proj_bias"):
        cross_selective_scan(**a, x_proj_bias=torch.zeros(4, 12))
    with pytest.raises(RuntimeError, match="step_size"):
        cross_selective_scan(**a, step_size=3)
    with pytest.raises(RuntimeError, match="delta_softplus"):
        cross_selective_scan(**a, delta_softplus=False)
    assert torch.cuda.is_initialized() == was
