"""The fused adaLN / gated residual of the trainable Mamba_block, host side, without a GPU: the C ABI of both builds of the library
(csrc/fd_adaln_train.hip), the argument checks of adaln_train and mamba_block_train, and the scratch of the new kernels."""
import os
import re
import shutil

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("fd_adaln_fwd_f32", "fd_adaln_bwd_ws_floats", "fd_adaln_bwd_f32", "fd_gate_res_fwd_f32", "fd_gate_res_bwd_ws_floats",
               "fd_gate_res_bwd_f32")
# (hw, C) of the nine Mamba_blocks of the architecture on a 512 x 512 slice: downs 0-3, middle, ups 0-3
BLOCKS = ((512 * 512, 64), (256 * 256, 64), (128 * 128, 128), (64 * 64, 256), (64 * 64, 512), (64 * 64, 512), (128 * 128, 256),
          (256 * 256, 128), (512 * 512, 64))


def test_new_entries_are_declared_and_exported():
    """declared in include/founddiff_hip.h, present in _lib's table, exported by both builds of the library"""
    from founddiff_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "founddiff_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b(int|int64_t) " + name + r"\(", hdr), name
        assert name in L.SIGNATURES, name
    for build in (L.BF16, L.F16):
        lib = build.lib()
        for name in NEW_SYMBOLS:
            assert hasattr(lib, name), name


def test_workspace_sizes():
    """positive multiples of 4 at the training shapes and at one pixel; an unsupported shape gets 0 floats"""
    from founddiff_amd import _lib as L
    for build in (L.BF16, L.F16):
        lib = build.lib()
        for hw, C in BLOCKS + ((1, 64),):
            n, m = lib.fd_adaln_bwd_ws_floats(2, hw, C), lib.fd_gate_res_bwd_ws_floats(2, hw, C)
            assert n > 0 and n % 4 == 0 and n >= 2 * 2 * C, (hw, C, n)
            assert m > 0 and m % 4 == 0 and m >= 2 * C, (hw, C, m)
        for bad in ((2, 64, 96), (2, 64, 32), (2, 64, 576), (0, 64, 64), (2, 0, 64)):
            assert lib.fd_adaln_bwd_ws_floats(*bad) == 0, bad
            assert lib.fd_gate_res_bwd_ws_floats(*bad) == 0, bad


def _raises(match, fn, *args):
    with pytest.raises(RuntimeError, match=match):
        fn(*args)


def test_functions_reject_before_cuda_is_initialised():
    """types and dtypes, then shapes, then devices: each with its message, and nothing touches the GPU"""
    from founddiff_amd import adaln_train as at
    was = torch.cuda.is_initialized()
    B, C = 2, 64
    x, y = torch.randn(B, 3, 5, C), torch.randn(B, 3, 5, C)
    gamma, beta = torch.ones(C), torch.zeros(C)
    shift, scale, gate = torch.randn(B, C), torch.randn(B, C), torch.randn(B, C)
    for fn in (at.adaln_fn, at.adaln_skip_fn):
        _raises("GPU", fn, x, gamma, beta, shift, scale, 1e-5)                                    # a CPU tensor
        _raises("GPU", fn, x, None, None, shift, scale, 1e-6)
        _raises("must be a tensor", fn, x, gamma, beta, None, scale, 1e-5)
        _raises("float32", fn, x.long(), gamma, beta, shift, scale, 1e-5)                         # an int tensor
        _raises("float32", fn, x, gamma, beta, shift, scale.int(), 1e-5)
        _raises("gamma and beta", fn, x, gamma, None, shift, scale, 1e-5)                         # a gamma without a beta
        _raises("gamma and beta", fn, x, None, beta, shift, scale, 1e-5)
        _raises("unsupported shape", fn, torch.randn(B, 3, 5, 32), torch.ones(32), torch.zeros(32), torch.randn(B, 32),
                torch.randn(B, 32), 1e-5)                                                         # C = 32
        _raises("unsupported shape", fn, torch.randn(B, 3, 5, 96), None, None, torch.randn(B, 96), torch.randn(B, 96), 1e-5)
        _raises("unsupported shape", fn, torch.randn(1, 1, 2, 576), None, None, torch.randn(1, 576), torch.randn(1, 576), 1e-5)
        _raises("inconsistent shapes", fn, x, gamma, beta, torch.randn(B, C + 1), scale, 1e-5)    # a (B, C + 1) shift
        _raises("inconsistent shapes", fn, x, gamma, beta, shift, torch.randn(B + 1, C), 1e-5)
        _raises("inconsistent shapes", fn, x, torch.ones(C + 1), torch.zeros(C + 1), shift, scale, 1e-5)
        _raises("inconsistent shapes", fn, x[0], gamma, beta, shift, scale, 1e-5)
    _raises("GPU", at.gate_residual_fn, x, y, gate)
    _raises("must be a tensor", at.gate_residual_fn, x, None, gate)
    _raises("float32", at.gate_residual_fn, x, y.long(), gate)
    _raises("float32", at.gate_residual_fn, x.double(), y, gate)
    _raises("unsupported shape", at.gate_residual_fn, torch.randn(B, 3, 5, 32), torch.randn(B, 3, 5, 32), torch.randn(B, 32))
    _raises("inconsistent shapes", at.gate_residual_fn, x, y, torch.randn(B, C + 1))
    _raises("inconsistent shapes", at.gate_residual_fn, x, y[:, :2], gate)
    assert torch.cuda.is_initialized() == was


def test_block_rejects_before_cuda_is_initialised():
    """mamba_block_forward: a CPU tensor, an int tensor, hidden_size 32 and a norm1 with a weight and no bias"""
    from founddiff_amd.mamba_block_train import MambaBlock
    was = torch.cuda.is_initialized()
    x, c, t = torch.randn(1, 64, 4, 4), torch.randn(1, 1, 256), torch.randn(1, 128)
    _raises("GPU", MambaBlock(64, 8, 128), x, c, t)
    _raises("float32", MambaBlock(64, 8, 128), x.long(), c, t)
    _raises("float32", MambaBlock(64, 8, 128), x, c, t.int())
    _raises("must be a tensor", MambaBlock(64, 8, 128), x, c, None)
    _raises("unsupported hidden_size", MambaBlock(32, 8, 128), torch.randn(1, 32, 4, 4), c, t)
    m = MambaBlock(64, 8, 128)
    m.norm1.bias = None
    _raises("both a weight and a bias", m, x, c, t)
    assert torch.cuda.is_initialized() == was


def test_new_kernels_use_no_scratch():
    """0 bytes of scratch per lane for every kernel of csrc/fd_adaln_train.hip, in both builds (hipcc's kernel-resource-usage
    remarks, founddiff_amd.build.resources())"""
    if not shutil.which("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    from founddiff_amd import build
    want = {"al_fwd_kernel", "al_bwd_kernel", "al_finish_kernel", "gr_fwd_kernel", "gr_bwd_kernel", "partial_sum_kernel"}
    for half in ("bf16", "fp16"):
        build.build(half=half)
        tab = build.resources(half).get("fd_adaln_train.hip")
        assert tab, "no resource remarks beside fd_adaln_train.hip's object: rebuild with build(force=True)"
        seen = {}
        for name, r in tab.items():
            assert r.get("scratch", 0) == 0, (half, name, r)
            m = re.search("|".join(sorted(want)), name)
            if m:
                seen[m.group(0)] = seen.get(m.group(0), 0) + 1
        assert set(seen) == want, set(seen) ^ want
        for name in ("al_fwd_kernel", "al_bwd_kernel", "gr_fwd_kernel", "gr_bwd_kernel"):
            assert seen[name] == 2, (name, seen)                         # one and two vectors per lane
