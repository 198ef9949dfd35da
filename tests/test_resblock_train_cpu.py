"""The trainable ResnetBlock's host side, without a GPU: the C ABI of both builds of the library (csrc/fd_resblock_train.hip),
resblock_train.ResnetBlock against the reference's captured state dicts, ws_weight against the oracle, the argument checks, and
the scratch of the new kernels."""
import os
import re
import shutil

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("fd_gn_silu_bwd_ws_floats", "fd_gn_silu_bwd_f32", "fd_conv3x3_wgrad_ws_floats", "fd_conv3x3_wgrad_f32")
# (name, H, W, Cin, Cout): the ten ResnetBlocks of a forward at 512 x 512
BLOCKS = (("down0", 512, 512, 64, 64), ("down1", 256, 256, 64, 64), ("down2", 128, 128, 128, 128), ("down3", 64, 64, 256, 256),
          ("mid", 64, 64, 512, 512), ("ups0", 64, 64, 768, 512), ("ups1", 128, 128, 384, 256), ("ups2", 256, 256, 192, 128),
          ("ups3", 512, 512, 128, 64), ("final", 512, 512, 128, 64))


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
    """the ten training shapes and the golden 48 -> 32 block are served; an unsupported shape gets 0 floats"""
    from founddiff_amd import _lib as L
    for build in (L.BF16, L.F16):
        lib = build.lib()
        for B, H, W, Cin, Cout in [(2,) + b[1:] for b in BLOCKS] + [(2, 3, 5, 48, 32)]:
            n = lib.fd_gn_silu_bwd_ws_floats(B, H * W, Cout, 8)
            assert n > 0 and n % 4 == 0 and n >= B * 3 * Cout + B * 8 * 2, (H, W, Cout, n)
            m = lib.fd_conv3x3_wgrad_ws_floats(B, H, W, Cin, Cout)
            assert m > 0 and m % 4 == 0, (H, W, Cin, Cout, m)
        # whole partial [Cout][9 Cin] blocks, one per split of the pixels: 256 (the cap) at down0, where there are only two output
        # tiles per split; a handful at ups0, which has 192; none for an image of one pixel tile
        assert lib.fd_conv3x3_wgrad_ws_floats(2, 512, 512, 64, 64) == 256 * 64 * 9 * 64
        assert lib.fd_conv3x3_wgrad_ws_floats(2, 64, 64, 768, 512) == 6 * 512 * 9 * 768
        assert lib.fd_conv3x3_wgrad_ws_floats(1, 8, 16, 64, 64) == 4
        for Cin, Cout, B in ((40, 64, 2), (64, 48, 2), (64, 576, 2), (64, 64, 0), (1040, 64, 2)):
            assert lib.fd_conv3x3_wgrad_ws_floats(B, 16, 16, Cin, Cout) == 0, (Cin, Cout, B)
        for C, B, hw, groups in ((48, 2, 256, 8), (576, 2, 256, 8), (64, 0, 256, 8), (64, 2, 0, 8), (64, 2, 256, 3), (32, 2, 256, 32)):
            assert lib.fd_gn_silu_bwd_ws_floats(B, hw, C, groups) == 0, (C, B, hw, groups)


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


def test_resnet_block_has_the_references_state_dict(golden):
    from founddiff_amd.resblock_train import ResnetBlock
    same, proj = _sub(golden, "rb_same."), _sub(golden, "rb_proj.")
    assert len(same) == 4 and len(proj) == 6
    m = ResnetBlock(32, 32)
    assert isinstance(m.res_conv, torch.nn.Identity)
    _same_state_dict(m, same)
    m = ResnetBlock(48, 32, time_emb_dim=128)
    assert sorted(m.state_dict()) == ["block1.norm.bias", "block1.norm.weight", "block1.proj.bias", "block1.proj.weight",
                                      "res_conv.bias", "res_conv.weight"]
    _same_state_dict(m, proj)
    assert ResnetBlock(64, 64, groups=4).block1.norm.num_groups == 4


def test_ws_weight_is_the_oracles(golden):
    from founddiff_amd.resblock_train import ws_weight
    from oracle import nets
    w = _sub(golden, "rb_proj.")["block1.proj.weight"].double()
    for eps in (1e-5, 1e-3):
        assert torch.equal(ws_weight(w, eps), nets.ws_weight(w, eps))
    got = ws_weight(w)
    assert float(got.mean(dim=(1, 2, 3)).abs().max()) < 1e-12 and abs(float(got.var(dim=(1, 2, 3), unbiased=False).mean()) - 1) < 1e-2


def _raises(match, fn, *args, **kw):
    with pytest.raises(RuntimeError, match=match):
        fn(*args, **kw)


def test_functions_reject_before_cuda_is_initialised():
    from founddiff_amd import resblock_train as rbt
    was = torch.cuda.is_initialized()
    x, w, v = torch.randn(1, 4, 4, 32), torch.randn(32, 32, 3, 3), torch.randn(32)
    f = rbt.block_core_fn
    _raises("GPU", f, x, w, v, v, v)
    _raises("GPU", f, x, w, v, v, v, torch.randn(1, 4, 4, 32))
    _raises("must be a tensor", f, x, w, None, v, v)
    _raises("must be a tensor", f, [1.0], w, v, v, v)
    _raises("must be a tensor", f, x, w, v, v, v, 3.0)
    _raises("float32", f, x.double(), w, v, v, v)
    _raises("float32", f, x, w, v, v.long(), v)
    # types and shapes are checked before devices
    _raises("inconsistent shapes", f, x[0], w, v, v, v)
    _raises("inconsistent shapes", f, x, torch.randn(32, 32, 5, 5), v, v, v)
    _raises("inconsistent shapes", f, x, torch.randn(32, 16, 3, 3), v, v, v)
    _raises("inconsistent shapes", f, x, w, torch.randn(16), v, v)
    _raises("inconsistent shapes", f, x, w, v, v, torch.randn(64))
    _raises("inconsistent shapes", f, x, w, v, v, v, torch.randn(1, 4, 4, 16))
    _raises("inconsistent shapes", f, x, w, v, v, v, torch.randn(2, 4, 4, 32))
    u = torch.randn(48)
    _raises("unsupported shape", f, torch.randn(1, 4, 4, 40), torch.randn(32, 40, 3, 3), v, v, v)             # Cin % 16
    _raises("unsupported shape", f, x, torch.randn(48, 32, 3, 3), u, u, u)                                    # Cout % 32
    _raises("unsupported shape", f, x, torch.randn(576, 32, 3, 3), *(torch.randn(576),) * 3)                  # Cout > 512
    _raises("unsupported shape", f, torch.randn(1, 2, 2, 1040), torch.randn(32, 1040, 3, 3), v, v, v)         # Cin > 1024
    _raises("unsupported shape", f, x, w, v, v, v, groups=3)
    _raises("unsupported shape", f, x, w, v, v, v, groups=16)                                                 # 2 channels per group
    assert torch.cuda.is_initialized() == was


def test_modules_reject_before_cuda_is_initialised():
    """a block1.proj that is not a 3 x 3 / padding 1 / stride 1 / dilation 1 / groups 1 convolution, a non-affine norm, a res_conv
    that is neither 1 x 1 nor Identity, unsupported channel counts, CPU tensors and inconsistent shapes raise RuntimeError before
    anything touches the GPU"""
    from founddiff_amd import resblock_train as rbt
    nn = torch.nn
    was = torch.cuda.is_initialized()
    x = torch.randn(1, 32, 4, 4)

    def module(dim=32, dim_out=32, proj=None, norm=None, **attrs):
        m = rbt.ResnetBlock(dim, dim_out)
        if proj is not None:
            m.block1.proj = proj
        if norm is not None:
            m.block1.norm = norm
        for k, v in attrs.items():
            setattr(m, k, v)
        return m
    _raises("GPU", module(), x)
    _raises("GPU", module(48, 32), torch.randn(1, 48, 4, 4))
    _raises("GPU", rbt.resnet_block_nhwc, module(), x.permute(0, 2, 3, 1))
    _raises("inconsistent shapes", module(48, 32), x)
    _raises("inconsistent shapes", rbt.resnet_block_nhwc, module(48, 32), x)
    _raises("inconsistent shapes", module(), x[0])
    _raises("must be a tensor", module(), None)
    _raises("float32", module(), x.double())
    _raises("3x3 convolution", module(proj=nn.Conv2d(32, 32, 5, padding=2)), x)
    _raises("3x3 convolution", module(proj=nn.Conv2d(32, 32, 3, padding=1, stride=2)), x)
    _raises("3x3 convolution", module(proj=nn.Conv2d(32, 32, 3, padding=1, groups=2)), x)
    _raises("3x3 convolution", module(proj=nn.Conv2d(32, 32, 3, padding=0)), x)
    _raises("3x3 convolution", module(proj=nn.Conv2d(32, 32, 3, padding=2, dilation=2)), x)
    _raises("3x3 convolution", module(proj=nn.Conv2d(32, 32, 3, padding=1, padding_mode="reflect")), x)
    _raises("affine GroupNorm", module(norm=nn.GroupNorm(8, 32, affine=False)), x)
    _raises("affine GroupNorm", module(norm=nn.BatchNorm2d(32)), x)
    _raises("1x1 convolution", module(res_conv=nn.Conv2d(32, 32, 3, padding=1)), x)
    _raises("1x1 convolution", module(res_conv=nn.ReLU()), x)
    _raises("inconsistent shapes", module(res_conv=nn.Conv2d(16, 32, 1)), x)
    _raises("inconsistent shapes", module(48, 32, res_conv=nn.Identity()), torch.randn(1, 48, 4, 4))
    _raises("inconsistent shapes", module(norm=nn.GroupNorm(8, 64)), x)
    _raises("unsupported shape", module(40, 32), torch.randn(1, 40, 4, 4))
    _raises("unsupported shape", module(32, 48), x)
    _raises("unsupported shape", module(32, 576), x)
    _raises("unsupported shape", module(norm=nn.GroupNorm(16, 32)), x)
    assert torch.cuda.is_initialized() == was


def test_new_kernels_use_no_scratch():
    """0 bytes of scratch per lane for every kernel of csrc/fd_resblock_train.hip in both builds (hipcc's kernel-resource-usage
    remarks, founddiff_amd.build.resources())"""
    if not shutil.which("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    from founddiff_amd import build
    want = {"partial_sum_kernel", "gsb_sums_kernel", "gsb_coef_kernel", "gsb_param_kernel", "gsb_dh_kernel",
            "tapcorr_kernelILi3ELi1ELi8ELi16ELi48E", "tapcorr_reduce_kernel"}
    for half in ("bf16", "fp16"):
        build.build(half=half)
        tab = build.resources(half).get("fd_resblock_train.hip")
        assert tab, "no resource remarks beside fd_resblock_train.hip's object: rebuild with build(force=True)"
        seen = set()
        for name, r in tab.items():
            assert r.get("scratch", 0) == 0, (half, name, r)
            m = re.search("|".join(sorted(want, key=len, reverse=True)), name)
            if m:
                seen.add(m.group(0))
        assert seen == want, seen ^ want
