"""The trainable resampling convolutions and the U-Net trunk, host side, without a GPU: the C ABI of both builds of the library
(csrc/fd_resample_train.hip), the three weight maps of founddiff_amd.resample_train against float64 torch, UnetTrunk's state dict
against arch.da_unet_spec, the argument checks, and the scratch of the new kernels."""
import os
import re
import shutil

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("fd_conv_sub2x_f32", "fd_corr4x4s2_ws_floats", "fd_corr4x4s2_f32")
# (name, coarse H, coarse W, P, Q) of fd_corr4x4s2_f32 for the six resampling convolutions of a forward at 512 x 512 (Down: coarse =
# dout, fine = x; Up: coarse = x, fine = dout) and for the two golden captures down.* / up.*
CORR = (("down0", 256, 256, 64, 64), ("down1", 128, 128, 128, 64), ("down2", 64, 64, 256, 128), ("ups0", 64, 64, 512, 256),
        ("ups1", 128, 128, 256, 128), ("ups2", 256, 256, 128, 64), ("golden down", 6, 5, 64, 32), ("golden up", 6, 5, 64, 32))


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
    """the six training shapes and the two golden ones are served; one pixel tile needs no partials; an unsupported shape gets 0"""
    from founddiff_amd import _lib as L
    for build in (L.BF16, L.F16):
        lib = build.lib()
        for name, H, W, P, Q in CORR:
            n = lib.fd_corr4x4s2_ws_floats(2, H, W, P, Q)
            assert n > 0 and n % 4 == 0, (name, n)
        # whole partial [P][16 Q] blocks, one per split of the coarse pixels: 256 (the cap) at down0, which has two output tiles;
        # 3 at ups0, where a partial is 8 MB and three are half of what the two activations take; none for one 4 x 8 pixel tile
        assert lib.fd_corr4x4s2_ws_floats(2, 256, 256, 64, 64) == 256 * 64 * 16 * 64
        assert lib.fd_corr4x4s2_ws_floats(2, 64, 64, 512, 256) == 3 * 512 * 16 * 256
        for name, H, W, P, Q in CORR:
            assert lib.fd_corr4x4s2_ws_floats(2, H, W, P, Q) <= max(4, 2 * H * W * (P + 4 * Q) // 2), name
        assert lib.fd_corr4x4s2_ws_floats(1, 4, 8, 64, 64) == 4
        for B, H, W, P, Q in ((2, 16, 16, 48, 64), (2, 16, 16, 64, 16), (2, 16, 16, 576, 64), (2, 16, 16, 64, 544), (0, 16, 16, 64, 64),
                              (2, 0, 16, 64, 64), (2, 16, 0, 64, 64)):
            assert lib.fd_corr4x4s2_ws_floats(B, H, W, P, Q) == 0, (B, H, W, P, Q)


def test_new_kernels_use_no_scratch():
    """0 bytes of scratch per lane for every kernel of csrc/fd_resample_train.hip in both builds (hipcc's kernel-resource-usage
    remarks, founddiff_amd.build.resources())"""
    if not shutil.which("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    from founddiff_amd import build
    want = {"sub2x_kernel", "tapcorr_kernelILi4ELi2ELi4ELi8ELi40E", "tapcorr_reduce_kernel"}
    for half in ("bf16", "fp16"):
        build.build(half=half)
        tab = build.resources(half).get("fd_resample_train.hip")
        assert tab, "no resource remarks beside fd_resample_train.hip's object: rebuild with build(force=True)"
        seen = set()
        for name, r in tab.items():
            assert r.get("scratch", 0) == 0, (half, name, r)
            m = re.search("|".join(sorted(want, key=len, reverse=True)), name)
            if m:
                seen.add(m.group(0))
        assert seen == want, seen ^ want


# ---- the weight maps, float64, Cin = Cout = 32, 6 x 5 ---------------------------------------------------------------------------------
def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def sub2x_einsum(x, w2, bias=None):
    """fd_conv_sub2x_f32's definition as einsums: x (B, H, W, C), w2 [N][4][2][2][C] -> (B, 2H, 2W, N)"""
    B, H, W, _ = x.shape
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    out = x.new_zeros(B, 2 * H, 2 * W, w2.shape[0])
    for a in range(2):
        for b in range(2):
            acc = 0
            for r in range(2):
                for s in range(2):
                    acc = acc + torch.einsum("bijc,nc->bijn", xp[:, a + r:a + r + H, b + s:b + s + W], w2[:, 2 * a + b, r, s])
            out[:, a::2, b::2] = acc
    return out if bias is None else out + bias


def corr_einsum(coarse, fine):
    """fd_corr4x4s2_f32's definition: coarse (B, H, W, P), fine (B, 2H, 2W, Q) -> g [P][4][4][Q]"""
    B, H, W, P = coarse.shape
    fp = F.pad(fine, (0, 0, 1, 1, 1, 1))
    g = coarse.new_zeros(P, 4, 4, fine.shape[3])
    for t in range(4):
        for u in range(4):
            g[:, t, u] = torch.einsum("bijp,bijq->pq", coarse, fp[:, t:t + 2 * H:2, u:u + 2 * W:2])
    return g


@pytest.fixture(scope="module")
def maps():
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 32, 6, 5, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(32, 32, 3, 3, generator=g, dtype=torch.float64, requires_grad=True)
    out = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, padding=1)
    dout = torch.randn(out.shape, generator=g, dtype=torch.float64)
    dx, dw = torch.autograd.grad(out, [x, w], dout)
    return x.detach(), w.detach(), out.detach(), dout, dx, dw


def test_the_subpixel_fold(maps):
    """nearest x2 -> conv3x3 == the sub-pixel form with sub2x_weight(up_weight_4x4(w))"""
    from founddiff_amd import resample_train as rt
    x, w, out, _, _, _ = maps
    w2 = rt.sub2x_weight(rt.up_weight_4x4(w))
    assert w2.shape == (32, 4, 2, 2, 32) and w2.is_contiguous()
    # the layout documented for weight_up2x: a = 0: r = 0 <- kh 0, r = 1 <- kh 1 + 2; a = 1: r = 0 <- kh 0 + 1, r = 1 <- kh 2
    rows = {(0, 0): (0,), (0, 1): (1, 2), (1, 0): (0, 1), (1, 1): (2,)}
    for (a, r), khs in rows.items():
        for (b, s), kws in rows.items():
            want = sum(w[:, :, kh, kw] for kh in khs for kw in kws)      # up to four terms, in another order than the fold's
            assert _rel(w2[:, 2 * a + b, r, s], want) < 1e-15, (a, b, r, s)
    e = _rel(sub2x_einsum(x.permute(0, 2, 3, 1), w2), out.permute(0, 2, 3, 1))
    print(f"[measured] sub-pixel fold: {e:.2e}")
    assert e < 1e-12


def test_the_folded_transposed_weight(maps):
    """Up's input gradient == the 4x4 / stride 2 / padding 1 convolution of dout with wd[c][t][u][n]"""
    from founddiff_amd import resample_train as rt
    _, w, _, dout, dx, _ = maps
    wd = rt.up_weight_4x4(w).permute(1, 2, 3, 0)
    # t = 0 <- kh 2, t = 1 <- kh 1 + 2, u = 2 <- kw 0 + 1, u = 3 <- kw 0
    assert torch.equal(wd[:, 0, 3], w[:, :, 2, 0].t())
    assert torch.equal(wd[:, 1, 2], ((w[:, :, 1, 0] + w[:, :, 2, 0]) + (w[:, :, 1, 1] + w[:, :, 2, 1])).t())
    e = _rel(F.conv2d(dout, wd.permute(0, 3, 1, 2), stride=2, padding=1), dx)
    print(f"[measured] wd: {e:.2e}")
    assert e < 1e-12


def test_the_unfold_of_g(maps):
    """Up's weight gradient == the unfold of g = corr(x, dout); Down's is g = corr(dout, x) as it is, and Down's input gradient
    is the sub-pixel form with the re-indexed 4x4 taps"""
    from founddiff_amd import resample_train as rt
    x, _, _, dout, _, dw = maps
    g = corr_einsum(x.permute(0, 2, 3, 1), dout.permute(0, 2, 3, 1))
    e = _rel(rt.up_weight_unfold(g.permute(3, 0, 1, 2)), dw)
    print(f"[measured] unfold of G: {e:.2e}")
    assert e < 1e-12
    gen = torch.Generator().manual_seed(12)
    xf = torch.randn(2, 32, 12, 10, generator=gen, dtype=torch.float64, requires_grad=True)
    w4 = torch.randn(32, 32, 4, 4, generator=gen, dtype=torch.float64, requires_grad=True)
    o = F.conv2d(xf, w4, stride=2, padding=1)
    do = torch.randn(o.shape, generator=gen, dtype=torch.float64)
    rdx, rdw = torch.autograd.grad(o, [xf, w4], do)
    e1 = _rel(corr_einsum(do.permute(0, 2, 3, 1), xf.detach().permute(0, 2, 3, 1)).permute(0, 3, 1, 2), rdw)
    e2 = _rel(sub2x_einsum(do.permute(0, 2, 3, 1), rt.sub2x_weight(w4.detach().transpose(0, 1))), rdx.permute(0, 2, 3, 1))
    print(f"[measured] Down: dweight {e1:.2e} dx {e2:.2e}")
    assert e1 < 1e-12 and e2 < 1e-12


# ---- the trunk --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mults", [(1, 2, 4, 8), (1, 2)])
def test_trunk_has_the_references_state_dict(mults):
    from founddiff_amd import arch, synth
    from founddiff_amd.unet_train import UnetTrunk
    spec = {k: v for k, v in arch.da_unet_spec(64, mults).items() if not k.startswith("dose_encoder.")}
    m = UnetTrunk(64, mults)
    own = m.state_dict()
    assert set(own) == set(spec), set(own) ^ set(spec)
    for k, v in spec.items():
        assert tuple(own[k].shape) == tuple(v), k
    sd = synth.synth_state_dict(spec, 3)
    m.load_state_dict(sd, strict=True)
    assert all(torch.equal(m.state_dict()[k], v) for k, v in sd.items())
    n = len(mults)
    assert [b[1].mamba.d_state for b in m.downs] == [4 * 2 ** i for i in range(n)]
    assert m.mid_attn.mamba.d_state == 32 and [b[1].mamba.d_state for b in m.ups] == [4 * 2 ** (3 - i) for i in range(n)]
    assert isinstance(m.downs[-1][2], torch.nn.Conv2d) and m.downs[-1][2].kernel_size == (3, 3)
    assert isinstance(m.ups[0][2], torch.nn.Sequential) and isinstance(m.ups[-1][2], torch.nn.Conv2d)
    # adaLN-Zero and the reference's prompt ~ U[0, 1)
    fresh = UnetTrunk(64, (1, 2))
    prompt = fresh.prompt.detach()
    assert not fresh.mid_attn.adaLN_modulation[-1].weight.any() and 0 <= float(prompt.min()) and float(prompt.max()) < 1


# ---- rejections ---------------------------------------------------------------------------------------------------------------------
def _raises(match, fn, *args, **kw):
    with pytest.raises(RuntimeError, match=match):
        fn(*args, **kw)


def test_functions_reject_before_cuda_is_initialised():
    from founddiff_amd import resample_train as rt
    was = torch.cuda.is_initialized()
    x, v = torch.randn(1, 4, 6, 32), torch.randn(32)
    w3, w4 = torch.randn(32, 32, 3, 3), torch.randn(32, 32, 4, 4)
    for f, w, other in ((rt.downsample_fn, w4, w3), (rt.upsample_fn, w3, w4), (rt.conv3x3_fn, w3, w4)):
        _raises("GPU", f, x, w, v)
        _raises("must be a tensor", f, x, w, None)
        _raises("must be a tensor", f, [1.0], w, v)
        _raises("float32", f, x.double(), w, v)
        _raises("float32", f, x, w, v.long())
        # types and shapes are checked before devices
        _raises("inconsistent shapes", f, x[0], w, v)
        _raises("inconsistent shapes", f, x, other, v)
        _raises("inconsistent shapes", f, x, w[:, :16], v)
        _raises("inconsistent shapes", f, x, w, torch.randn(16))
        k = w.shape[-1]
        _raises("unsupported shape", f, torch.randn(1, 4, 6, 48), torch.randn(32, 48, k, k), v)                 # Cin % 32
        _raises("unsupported shape", f, x, torch.randn(48, 32, k, k), torch.randn(48))                          # Cout % 32
        _raises("unsupported shape", f, x, torch.randn(544, 32, k, k), torch.randn(544))                        # Cout > 512
        _raises("unsupported shape", f, torch.randn(1, 2, 2, 544), torch.randn(32, 544, k, k), v)               # Cin > 512
    _raises("unsupported shape", rt.downsample_fn, torch.randn(1, 5, 6, 32), w4, v)                             # odd H
    _raises("unsupported shape", rt.downsample_fn, torch.randn(1, 4, 7, 32), w4, v)                             # odd W
    assert torch.cuda.is_initialized() == was


def test_modules_reject_before_cuda_is_initialised():
    """resample_nhwc: anything but the reference's three module forms, a missing bias, unsupported channel counts, CPU tensors and
    inconsistent shapes raise RuntimeError before anything touches the GPU; so do unet_forward's own checks"""
    from founddiff_amd import resample_train as rt
    from founddiff_amd.unet_train import UnetTrunk
    nn = torch.nn
    was = torch.cuda.is_initialized()
    x = torch.randn(1, 4, 6, 32)
    up = lambda conv, **kw: nn.Sequential(nn.Upsample(**(kw or dict(scale_factor=2, mode="nearest"))), conv)
    f = rt.resample_nhwc
    for m in (nn.Conv2d(32, 64, 4, 2, 1), up(nn.Conv2d(32, 64, 3, padding=1)), nn.Conv2d(32, 64, 3, padding=1)):
        _raises("GPU", f, m, x)
        _raises("inconsistent shapes", f, m, x[0])
        _raises("inconsistent shapes", f, m, torch.randn(1, 4, 6, 64))
        _raises("must be a tensor", f, m, None)
        _raises("float32", f, m, x.double())
    _raises("unsupported shape", f, nn.Conv2d(32, 64, 4, 2, 1), torch.randn(1, 5, 6, 32))
    for m in (nn.Conv2d(32, 48, 4, 2, 1), up(nn.Conv2d(32, 48, 3, padding=1)), nn.Conv2d(32, 544, 3, padding=1)):
        _raises("unsupported shape", f, m, x)
    for m in (nn.Conv2d(32, 64, 4, 2, 1, bias=False), up(nn.Conv2d(32, 64, 3, padding=1, bias=False)),
              nn.Conv2d(32, 64, 3, padding=1, bias=False)):
        _raises("must have a bias", f, m, x)
    for m in (nn.Conv2d(32, 64, 4, 2, 0), nn.Conv2d(32, 64, 4, 1, 1), nn.Conv2d(32, 64, 3, padding=0), nn.Conv2d(32, 64, 5, padding=2),
              nn.Conv2d(32, 64, 3, padding=1, groups=2), nn.Conv2d(32, 64, 3, padding=2, dilation=2),
              nn.Conv2d(32, 64, 3, padding=1, padding_mode="reflect"), nn.Conv2d(32, 64, 3, 2, 1),
              up(nn.Conv2d(32, 64, 3, padding=1), scale_factor=2, mode="bilinear"),
              up(nn.Conv2d(32, 64, 3, padding=1), scale_factor=4, mode="nearest"), up(nn.Conv2d(32, 64, 3, padding=1), size=(8, 8)),
              up(nn.Conv2d(32, 64, 4, 2, 1)), nn.Sequential(nn.Conv2d(32, 64, 3, padding=1)), nn.ReLU(), None):
        _raises("the module must be", f, m, x)
    trunk = UnetTrunk(64, (1, 2))
    x2, t, d, c = torch.randn(1, 2, 16, 16), torch.rand(1), torch.randn(1, 1024), torch.randn(1, 1, 256)
    _raises("GPU", trunk, x2, t, d, c)
    _raises("must be a tensor", trunk, x2, t, None, c)
    assert torch.cuda.is_initialized() == was
