"""The trainable TransposedAttention / Mamba_block's host side, without a GPU: the C ABI of both builds of the library
(csrc/fd_tattn_train.hip, fd_dwconv3x3_bwd_f32 of csrc/fd_ss2d_train.hip), tattn_train.TransposedAttention and
mamba_block_train.MambaBlock against the reference's captured state dicts, the argument checks, and the scratch of the new
kernels."""
import os
import re
import shutil

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("fd_chan_attn_fwd_ws_floats", "fd_chan_attn_fwd_f32", "fd_chan_attn_bwd_ws_floats", "fd_chan_attn_bwd_f32",
               "fd_dwconv3x3_bwd_ws_floats", "fd_dwconv3x3_bwd_f32")


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
    """the training shapes are served; an unsupported shape gets 0 floats"""
    from founddiff_amd import _lib as L
    for build in (L.BF16, L.F16):
        lib = build.lib()
        for hw, C in ((512 * 512, 64), (256 * 256, 64), (128 * 128, 128), (64 * 64, 256), (64 * 64, 512), (1, 64)):
            nblk = (hw + (1024 if hw >= 65536 else 256) - 1) // (1024 if hw >= 65536 else 256)
            n = lib.fd_chan_attn_fwd_ws_floats(2, hw, C)
            assert n % 4 == 0 and n >= 2 * (C // 32) * nblk * 1088, (hw, C, n)
            m = lib.fd_chan_attn_bwd_ws_floats(2, hw, C)
            assert m % 4 == 0 and m >= n + 2 * (C // 32) * 1089, (hw, C, m)
        for bad in ((2, 64, 96), (2, 64, 32), (2, 64, 576), (0, 64, 64), (2, 0, 64)):
            assert lib.fd_chan_attn_fwd_ws_floats(*bad) == 0, bad
            assert lib.fd_chan_attn_bwd_ws_floats(*bad) == 0, bad
        n = lib.fd_dwconv3x3_bwd_ws_floats(2, 512, 512, 192)
        assert n > 0 and n % 4 == 0 and n >= 10 * 192 + 9 * 192
        assert lib.fd_dwconv3x3_bwd_ws_floats(2, 64, 64, 1536) > 0
        assert lib.fd_dwconv3x3_bwd_ws_floats(2, 512, 512, 96) == 0
        assert lib.fd_dwconv3x3_bwd_ws_floats(0, 512, 512, 192) == 0


def _sub(golden, prefix):
    return {k[len(prefix):]: v for k, v in golden("modules").weights(prefix).items()}


def _same_state_dict(m, sd):
    own = m.state_dict()
    assert set(own) == set(sd), set(own) ^ set(sd)
    for k, v in sd.items():
        assert tuple(own[k].shape) == tuple(v.shape), k
    m.load_state_dict(sd, strict=True)
    for k, v in sd.items():
        assert torch.equal(m.state_dict()[k], v), k


def test_transposed_attention_has_the_references_state_dict(golden):
    from founddiff_amd.tattn_train import TransposedAttention
    sd = _sub(golden, "tattn.")
    assert len(sd) == 4
    _same_state_dict(TransposedAttention(64, 2), sd)
    m = TransposedAttention(64, 2, bias=True)
    assert sorted(k for k in m.state_dict() if k.endswith("bias")) == ["project_out.bias", "qkv.bias", "qkv_dwconv.bias"]
    assert torch.equal(m.temperature, torch.ones(2, 1, 1))


def test_mamba_block_has_the_references_state_dict(golden):
    from founddiff_amd.mamba_block_train import MambaBlock
    sd = _sub(golden, "mamba_c64.")
    assert len(sd) == 20                           # norm1 2, mamba 12, adaLN_modulation 2, attn_blk 4; norm2 has no parameters
    m = MambaBlock(64, 8, 128)
    lin = m.adaLN_modulation[-1]
    assert not lin.weight.any() and not lin.bias.any()          # adaLN-Zero
    assert m.norm2.eps == 1e-6 and m.norm2.weight is None and m.cross is False
    _same_state_dict(m, sd)


def _raises(match, fn, *args):
    with pytest.raises(RuntimeError, match=match):
        fn(*args)


def test_functions_reject_before_cuda_is_initialised():
    from founddiff_amd import tattn_train as tat
    was = torch.cuda.is_initialized()
    qkv, temp = torch.randn(1, 4, 4, 192), torch.ones(2, 1, 1)
    w = torch.randn(192, 1, 3, 3)
    _raises("GPU", tat.chan_attn_fn, qkv, temp)
    _raises("GPU", tat.chan_attn_fn, qkv, torch.ones(2))
    _raises("GPU", tat.tattn_core_fn, qkv, w, None, temp)
    _raises("GPU", tat.tattn_core_fn, qkv, w, torch.zeros(192), temp)
    _raises("must be a tensor", tat.chan_attn_fn, qkv, None)
    _raises("must be a tensor", tat.tattn_core_fn, qkv, None, None, temp)
    _raises("float32", tat.chan_attn_fn, qkv.double(), temp)
    _raises("float32", tat.tattn_core_fn, qkv, w, None, temp.long())
    # types and shapes are checked before devices
    _raises("inconsistent shapes", tat.chan_attn_fn, qkv[0], temp)
    _raises("inconsistent shapes", tat.chan_attn_fn, torch.randn(1, 4, 4, 200), temp)
    _raises("inconsistent shapes", tat.chan_attn_fn, qkv, torch.ones(3))              # heads * 32 != dim
    _raises("inconsistent shapes", tat.chan_attn_fn, qkv, torch.ones(1, 2, 1))
    _raises("inconsistent shapes", tat.tattn_core_fn, qkv, torch.randn(192, 1, 5, 5), None, temp)
    _raises("inconsistent shapes", tat.tattn_core_fn, qkv, torch.randn(96, 1, 3, 3), None, temp)
    _raises("inconsistent shapes", tat.tattn_core_fn, qkv, w, torch.zeros(64), temp)
    _raises("unsupported shape", tat.chan_attn_fn, torch.randn(1, 4, 4, 96), torch.ones(1))        # dim 32
    _raises("unsupported shape", tat.chan_attn_fn, torch.randn(1, 4, 4, 288), torch.ones(3))       # dim 96
    _raises("unsupported shape", tat.chan_attn_fn, torch.randn(1, 2, 2, 3 * 576), torch.ones(18))  # dim 576 > 512
    _raises("unsupported shape", tat.tattn_core_fn, torch.randn(1, 4, 4, 96), torch.randn(96, 1, 3, 3), None, torch.ones(1))
    assert torch.cuda.is_initialized() == was


def test_modules_reject_before_cuda_is_initialised():
    """num_heads * 32 != dim, dim % 64 != 0, dim > 512, a qkv_dwconv that is not a depthwise 3 x 3 with padding 1 / stride 1 /
    dilation 1, cross=True, CPU tensors and inconsistent shapes raise RuntimeError before anything touches the GPU"""
    from founddiff_amd import tattn_train as tat
    from founddiff_amd.mamba_block_train import MambaBlock
    nn = torch.nn
    was = torch.cuda.is_initialized()
    x = torch.randn(1, 64, 4, 4)

    def module(dim=64, heads=2, **attrs):
        m = tat.TransposedAttention(dim, heads)
        for k, v in attrs.items():
            setattr(m, k, v)
        return m
    _raises("GPU", module(), x)
    _raises("GPU", tat.transposed_attention_nhwc, module(), x.permute(0, 2, 3, 1))
    _raises("inconsistent shapes", module(), x.permute(0, 2, 3, 1))
    _raises("inconsistent shapes", tat.transposed_attention_nhwc, module(), x)
    _raises("must be a tensor", module(), None)
    _raises("heads of 32", module(heads=1), x)
    _raises("heads of 32", module(heads=4), x)
    _raises("unsupported shape", module(32, 1), torch.randn(1, 32, 4, 4))
    _raises("unsupported shape", module(96, 3), torch.randn(1, 96, 4, 4))
    _raises("unsupported shape", module(576, 18), torch.randn(1, 576, 2, 2))
    _raises("depthwise 3x3", module(qkv_dwconv=nn.Conv2d(192, 192, 5, padding=2, groups=192, bias=False)), x)
    _raises("depthwise 3x3", module(qkv_dwconv=nn.Conv2d(192, 192, 3, padding=1, bias=False)), x)
    _raises("depthwise 3x3", module(qkv_dwconv=nn.Conv2d(192, 192, 3, padding=0, groups=192, bias=False)), x)
    _raises("depthwise 3x3", module(qkv_dwconv=nn.Conv2d(192, 192, 3, padding=1, stride=2, groups=192, bias=False)), x)
    _raises("depthwise 3x3", module(qkv_dwconv=nn.Conv2d(192, 192, 3, padding=1, dilation=2, groups=192, bias=False)), x)
    c, t = torch.randn(1, 1, 256), torch.randn(1, 128)
    _raises("GPU", MambaBlock(64, 8, 128), x, c, t)
    _raises("inconsistent shapes", MambaBlock(64, 8, 128), x.permute(0, 2, 3, 1), c, t)
    _raises("inconsistent shapes", MambaBlock(64, 8, 128), x, c, torch.randn(2, 128))
    _raises("unsupported hidden_size", MambaBlock(32, 8, 128), torch.randn(1, 32, 4, 4), c, t)
    m = MambaBlock(64, 8, 128)
    m.cross = True
    _raises("cross=True", m, x, c, t)
    assert torch.cuda.is_initialized() == was


def test_new_kernels_use_no_scratch():
    """0 bytes of scratch per lane for every kernel of csrc/fd_tattn_train.hip and both forms of the depthwise-conv backward, in
    both builds (hipcc's kernel-resource-usage remarks, founddiff_amd.build.resources())"""
    if not shutil.which("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    from founddiff_amd import build
    want = {"ta_gram_kernel", "ta_reduce_kernel", "ta_softmax_kernel", "ta_apply_kernel", "ta_bwd_small_kernel", "ta_dtemp_kernel",
            "ta_bwd_stream_kernel"}
    for half in ("bf16", "fp16"):
        build.build(half=half)
        res = build.resources(half)
        tab = res.get("fd_tattn_train.hip")
        assert tab, "no resource remarks beside fd_tattn_train.hip's object: rebuild with build(force=True)"
        seen = set()
        for name, r in tab.items():
            assert r.get("scratch", 0) == 0, (half, name, r)
            m = re.search("|".join(sorted(want)), name)
            if m:
                seen.add(m.group(0))
        assert seen == want, seen ^ want
        dwb = {n: r for n, r in res["fd_ss2d_train.hip"].items() if "dwb_pre_kernel" in n}
        assert len(dwb) == 2                         # with and without the SiLU
        for name, r in dwb.items():
            assert r.get("scratch", 0) == 0, (half, name, r)
