"""GPU parity of the individual HIP kernels (called through the C ABI) against plain fp32
PyTorch-CPU restatements of the same op.  fp32 mode must agree to ~1e-5 (exact-f32 MFMA);
bf16 mode is compared with inputs pre-rounded to bf16 so only accumulation order and the
output rounding differ."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from conftest import HB, gate2x, rel_err, use_half_build
from scan_cases import scan_reference

pytestmark = pytest.mark.gpu

MODES = [("fp32", 2e-5), ("bf16", 1.2e-2)]
# every (d_inner, d_state, dt_rank) of the shipped architecture (downs.0/ups.3, downs.1, downs.2,
# downs.3, mid/ups.0, ups.1, ups.2) at small images, plus shapes of the tiny models
BLOCK_SHAPES = [(128, 4, 4, 16, 24), (128, 8, 4, 16, 16), (256, 16, 8, 16, 16), (512, 32, 16, 16, 8), (1024, 32, 32, 8, 16),
                (512, 16, 16, 16, 8), (256, 8, 8, 16, 16)]


@pytest.fixture(scope="module", params=["bf16-build", "fp16-build"], autouse=True)
def half_build(request):
    """every test of this module once per build of the library (conftest.use_half_build)"""
    use_half_build(request.param == "fp16-build")
    yield request.param
    use_half_build(False)


@pytest.fixture(autouse=True)
def _default_build_only(request, half_build):
    """the fp32-storage, split and fp8 modes belong to the default build: not repeated on the binary16 one"""
    if half_build == "fp16-build":
        mode = getattr(request.node, "callspec", None) and request.node.callspec.params.get("mode")
        name = request.node.name
        if mode in ("fp32", "fp32s", "fp8") or any(k in name for k in ("fp8", "fp32", "split", "reference_signature", "long_sequence",
                                                                       "integration_recipe")):
            pytest.skip("default build only")


def bare_engine_class():
    """DAEngine without weights: the op wrappers (conv, linear, ...) over the library build that is current"""
    from founddiff_amd import _lib as L
    from founddiff_amd.engine import DAEngine
    L.lib()

    class Bare(DAEngine):
        def __init__(self, mode):
            from founddiff_amd.engine import _T
            self.mode = mode
            self.dt, self.tdt = _T[mode]
            self.hip = L.BF16                     # (conftest.use_half_build: the binary16 build in the fp16 flavour)
            self.dev = torch.device("cuda")
            self.buf = {}
            self.f32_split = int(mode == "fp32s")
    return Bare


@pytest.fixture(scope="module")
def eng_factory(half_build):
    return bare_engine_class()


def nhwc(x, tdt):
    return x.permute(0, 2, 3, 1).contiguous().to("cuda", tdt)


def nchw(x):
    return x.float().cpu().permute(0, 3, 1, 2).contiguous()


def rq(x, mode):
    return x.to(HB.t).float() if mode == "bf16" else x


# 'fp32s': fp32 storage, split-bf16 contraction (3 bf16 MFMAs per product, ~2^-16): the engine of a bf16 loop's last step
@pytest.mark.parametrize("mode,tol", MODES + [("fp32s", 1e-4)])
@pytest.mark.parametrize("cfg", [
    dict(cin=64, cout=64, k=3, s=1, p=1, hw=(24, 20)),
    dict(cin=64, cout=128, k=4, s=2, p=1, hw=(16, 24)),
    dict(cin=8, cout=32, k=7, s=1, p=3, hw=(20, 20)),
    dict(cin=96, cout=40, k=1, s=1, p=0, hw=(9, 13)),
    dict(cin=128, cout=200, k=3, s=1, p=1, hw=(8, 8)),
    dict(cin=32, cout=64, k=3, s=1, p=1, hw=(6, 10), up=True),
])
def test_conv(eng_factory, mode, tol, cfg):
    from founddiff_amd.engine import ConvW
    e = eng_factory(mode)
    torch.manual_seed(0)
    B = 2
    H, W = cfg["hw"]
    x = rq(torch.randn(B, cfg["cin"], H, W), mode)
    w = rq(torch.randn(cfg["cout"], cfg["cin"], cfg["k"], cfg["k"]) / (cfg["cin"] * cfg["k"] ** 2) ** 0.5, mode)
    b = torch.randn(cfg["cout"])
    xin = F.interpolate(x, scale_factor=2, mode="nearest") if cfg.get("up") else x
    ref = F.conv2d(xin, w, b, stride=cfg["s"], padding=cfg["p"])
    cw = ConvW(w, b, e.dev, e.tdt)
    out = torch.empty(B, ref.shape[2], ref.shape[3], cfg["cout"], device="cuda", dtype=e.tdt)
    e.conv(cw, nhwc(x, e.tdt), B, H, W, out, stride=cfg["s"], pad=cfg["p"], upsample=cfg.get("up", False))
    torch.cuda.synchronize()
    assert rel_err(nchw(out), ref) < tol


@pytest.mark.parametrize("cfg", [
    dict(c0=512, c1=0, cout=2048, hw=(64, 64), epi="silu_split", kid=7),       # in_proj of the 512-channel blocks
    dict(c0=1024, c1=0, cout=512, hw=(64, 64), epi="gate_res", kid=7),         # out_proj: gated residual
    dict(c0=256, c1=0, cout=768, hw=(64, 64), epi="none", kid=7),              # qkv of the 256-channel block: 3 column tiles
    dict(c0=256, c1=0, cout=768, hw=(128, 128), epi="none", kid=7),            # qkv at 128x128: 6 tiles per workgroup, 3 column tiles
    dict(c0=512, c1=0, cout=256, hw=(128, 128), epi="gate_res", kid=7),        # out_proj at 128x128: one column tile
    dict(c0=256, c1=192, cout=328, hw=(60, 52), epi="none", kid=5),            # two sources, ragged M and N tiles
])
def test_pointwise_gemm_256_tile(eng_factory, cfg):
    """1x1 convolutions of the 64x64 / 128x128 levels at batch 8: the persistent 256x256 pointwise GEMM with deferred
    stores (fd_conv_kernel_id == 7, fd_pwgemm.hip) and the 256x256 tile of the generic kernel (== 5) against the fp32
    composition, with the pointwise epilogues they use; repeated launches reproduce the first one bit for bit, and the
    persistent kernel gives the SAME BITS as the generic tile (same K order per output element: the same problem posed
    with its K axis split over two sources is not eligible for the persistent kernel and runs on the generic one)."""
    from founddiff_amd import _lib as L
    from founddiff_amd.engine import ConvW
    e = eng_factory("bf16")
    torch.manual_seed(5)
    B, (H, W) = 8, cfg["hw"]
    c0, c1, cout = cfg["c0"], cfg["c1"], cfg["cout"]
    bf = lambda t: t.to(HB.t).float()
    a = bf(torch.randn(B, H, W, c0))
    a1 = bf(torch.randn(B, H, W, c1)) if c1 else None
    w = bf(torch.randn(cout, c0 + c1) / (c0 + c1) ** 0.5)
    bias = torch.randn(cout)
    xin = torch.cat((a, a1), -1) if c1 else a
    ref = F.linear(xin, w, bias)
    cw = ConvW(w, bias, e.dev, e.tdt)
    out = torch.zeros(B, H, W, cout, device="cuda", dtype=HB.t)
    kw = dict(c0=c0)
    if c1:
        kw.update(in1=a1.cuda().to(HB.t), c1=c1)
    if cfg["epi"] == "silu_split":
        kw.update(epi=L.EPI_SILU_SPLIT, split=cout // 2)
        ref[..., cout // 2:] = F.silu(ref[..., cout // 2:])
    elif cfg["epi"] == "gate_res":
        res = bf(torch.randn(B, H, W, cout))
        gate = torch.randn(B, cout)
        kw.update(epi=L.EPI_GATE_RES, res=res.cuda().to(HB.t), gate=gate.cuda(), gate_ld=cout)
        ref = res + gate[:, None, None, :] * ref
    ad = a.cuda().to(HB.t)
    assert e.conv(cw, ad, B, H, W, out, probe="kid", **kw) == cfg["kid"]
    e.conv(cw, ad, B, H, W, out, **kw)
    torch.cuda.synchronize()
    assert rel_err(out.float().cpu(), ref) < 6e-3
    first = out.clone()
    for _ in range(8):
        out.zero_()
        e.conv(cw, ad, B, H, W, out, **kw)
        torch.cuda.synchronize()
        assert torch.equal(out, first)
    if cfg["kid"] == 7:
        h0 = c0 // 2
        kw2 = dict(kw, c0=h0, in1=ad[..., h0:].contiguous(), c1=c0 - h0)
        a0 = ad[..., :h0].contiguous()
        assert e.conv(cw, a0, B, H, W, out, probe="kid", **kw2) == 5
        out.zero_()
        e.conv(cw, a0, B, H, W, out, **kw2)
        torch.cuda.synchronize()
        # (on the binary16 build too: csrc/fd_common.h fd_cvt_h -- without it the compiler's v_fma_mixlo_f16 fold in ONE of the two
        #  kernels made 6e-5 of the elements differ by a binary16 ulp)
        assert torch.equal(out, first)


@pytest.mark.parametrize("mode,tol", MODES)
def test_conv_concat_slices_epilogues(eng_factory, mode, tol):
    from founddiff_amd import _lib as L
    from founddiff_amd.engine import ConvW
    e = eng_factory(mode)
    torch.manual_seed(1)
    B, H, W = 2, 12, 10
    a, b2 = rq(torch.randn(B, 32, H, W), mode), rq(torch.randn(B, 16, H, W), mode)
    w = rq(torch.randn(64, 48, 3, 3) / 20, mode)
    bias = torch.randn(64)
    ref = F.conv2d(torch.cat((a, b2), 1), w, bias, padding=1)
    cw = ConvW(w, bias, e.dev, e.tdt)
    out = torch.empty(B, H, W, 64, device="cuda", dtype=e.tdt)
    mt = L.lib().fd_conv_mtiles(H, W)
    part = torch.zeros(B, mt, 64, 2, device="cuda")
    e.conv(cw, nhwc(a, e.tdt), B, H, W, out, c0=32, in1=nhwc(b2, e.tdt), c1=16, stats=part)
    torch.cuda.synchronize()
    assert rel_err(nchw(out), ref) < tol
    s = part.sum(1).cpu()
    assert rel_err(s[..., 0], ref.sum((2, 3))) < (5e-3 if mode == "bf16" else 1e-4)
    assert rel_err(s[..., 1], (ref ** 2).sum((2, 3))) < (5e-3 if mode == "bf16" else 1e-4)
    # silu split + strided / offset output + fp32 out
    wide = torch.zeros(B, H, W, 96, device="cuda", dtype=torch.float32)
    e.conv(cw, nhwc(a, e.tdt), B, H, W, wide, c0=32, in1=nhwc(b2, e.tdt), c1=16, ldo=96, offo=16, out_f32=True,
           epi=L.EPI_SILU_SPLIT, split=32)
    torch.cuda.synchronize()
    r2 = ref.clone()
    r2[:, 32:] = F.silu(r2[:, 32:])
    assert rel_err(nchw(wide[..., 16:80]), r2) < (4e-3 if mode == "bf16" else 2e-5)
    assert float(wide[..., :16].abs().max()) == 0 and float(wide[..., 80:].abs().max()) == 0
    # gated residual with per-batch weights, A operand = channel slice of a wider tensor
    big = rq(torch.randn(B, 96, H, W), mode)
    wb = rq(torch.randn(B, 32, 32) / 6, mode)
    res = rq(torch.randn(B, 32, H, W), mode)
    gate = torch.randn(B, 50)
    refg = torch.stack([F.conv2d(big[i:i + 1, 64:96], wb[i][:, :, None, None])[0] for i in range(B)])
    refg = res + gate[:, 7:39, None, None] * refg
    og = torch.empty(B, H, W, 32, device="cuda", dtype=e.tdt)
    gd = gate.cuda()
    e.conv(None, nhwc(big, e.tdt), B, H, W, og, c0=32, ld0=96, off0=64, weight=wb.to("cuda", e.tdt),
           w_batch_stride=32 * 32, bias=None, Cout=32, KH=1, KW=1, epi=L.EPI_GATE_RES, res=nhwc(res, e.tdt),
           gate=C.c_void_p(gd.data_ptr() + 7 * 4), gate_ld=50)
    torch.cuda.synchronize()
    assert rel_err(nchw(og), refg) < tol


def test_row_gemm_final_conv_ddim_epilogue(eng_factory):
    """EPI_GNSILU_ADD_FINAL of the streaming row-GEMM: res_conv + SiLU(GN(h)) + final_conv (64 -> 1) + the DDIM
    update in one epilogue (src/DADiff.py:733-740, 1203-1206, 1317-1318, 1344) against the unfused sequence
    EPI_GNSILU_ADD -> fd_final_conv1 -> fd_res_ddim_step on the same inputs, and against the fp32 composition."""
    from founddiff_amd import _lib as L
    from founddiff_amd.engine import ConvW
    e = eng_factory("bf16")
    torch.manual_seed(41)
    B, H, W, Ci, Co = 2, 128, 136, 128, 64                   # >= 16384 px: the row-GEMM path
    x = rq(torch.randn(B, Ci, H, W), "bf16")
    h = rq(torch.randn(B, Co, H, W) * 2 + 0.5, "bf16")
    w = rq(torch.randn(Co, Ci, 1, 1) / Ci ** 0.5, "bf16")
    bias, g, bb = torch.randn(Co), torch.randn(Co), torch.randn(Co)
    fw, fb = torch.randn(Co) / 8, 0.3
    hv = h.reshape(B, 8, -1)
    mr = torch.stack([hv.mean(-1), torch.rsqrt(hv.var(-1, unbiased=False) + 1e-5)], -1).contiguous().cuda()
    img, xin = torch.randn(B, 1, H, W).cuda(), torch.randn(B, 1, H, W).cuda().clamp(-1, 1)
    cw = ConvW(w, bias, e.dev, e.tdt)
    xd, hd = nhwc(x, e.tdt), nhwc(h, e.tdt)
    xa, xb = xd[..., :64].contiguous(), xd[..., 64:].contiguous()
    gd, bd, fwd = g.cuda(), bb.cuda(), fw.cuda()
    kw = dict(c0=64, in1=xb, c1=64, h=hd, gn=mr, gamma=gd, beta=bd, groups=8)
    # unfused
    o64 = torch.empty(B, H, W, Co, device="cuda", dtype=e.tdt)
    e.conv(cw, xa, B, H, W, o64, epi=L.EPI_GNSILU_ADD, **kw)
    mo0 = torch.empty(B, 1, H, W, device="cuda")
    fbd = torch.tensor([fb], device="cuda")
    L.call("fd_final_conv1", e.dt, o64.data_ptr(), fwd.data_ptr(), fbd.data_ptr(), mo0.data_ptr(), B * H * W, Co, e.stream)
    ref32 = (F.conv2d(x, w, bias) + F.silu(F.group_norm(h, 8, g, bb, 1e-5)))
    ref_mo = (ref32 * fw[None, :, None, None]).sum(1, keepdim=True) + fb
    for mode, lastf, alpha in ((0, 0, 0.0), (1, 0, 0.037), (1, 1, 0.0)):
        mo1 = torch.full((B, 1, H, W), float("nan"), device="cuda")
        im1, im0 = img.clone(), img.clone()
        fin = dict(w=fwd, b=fb, out=mo1, mode=mode, last=lastf, alpha=alpha, img=im1, xin=xin)
        assert e.conv(cw, xa, B, H, W, mo1, epi=L.EPI_GNSILU_ADD_FINAL, probe=True, fin=fin, **kw)
        e.conv(cw, xa, B, H, W, mo1, epi=L.EPI_GNSILU_ADD_FINAL, fin=fin, **kw)
        torch.cuda.synchronize()
        assert float((mo1 - mo0).abs().max()) < 2e-5 * float(mo0.abs().max()) + 1e-5      # same rounding points: fp32 sum order
        assert rel_err(mo1.cpu(), ref_mo) < 1e-2
        if mode == 1:
            L.call("fd_res_ddim_step", mo0.data_ptr(), im0.data_ptr(), xin.data_ptr(), None, alpha, 0.0, lastf, im0.data_ptr(),
                   im0.numel(), e.stream)
            torch.cuda.synchronize()
            assert float((im1 - im0).abs().max()) < 1e-4
        else:
            assert torch.equal(im1, img)


@pytest.mark.parametrize("mode,tol", MODES)
def test_xproj_directions(eng_factory, mode, tol):
    """x_proj as 4 stride-2 1x1 convs with sub-grid origins == einsum over EfficientScan output."""
    e = eng_factory(mode)
    torch.manual_seed(2)
    B, D, H, W, CD = 2, 64, 8, 12, 12
    x = rq(torch.randn(B, D, H, W), mode)
    xw = rq(torch.randn(4, CD, D) / 8, mode)
    out = torch.empty(4, B, (H // 2) * (W // 2), CD, device="cuda", dtype=torch.float32)
    e.conv(None, nhwc(x, e.tdt), B, H, W, out, c0=D, weight=xw.to("cuda", e.tdt), bias=None, Cout=CD, KH=1, KW=1,
           stride=2, pad=0, ndir=4, w_dir_stride=CD * D, out_dir_stride=B * (H // 2) * (W // 2) * CD,
           out_f32=True, OH=H // 2, OW=W // 2)
    torch.cuda.synchronize()
    for k in range(4):
        sub = x[:, :, (k & 1)::2, (k >> 1)::2]                      # (B,D,H/2,W/2)
        ref = torch.einsum("bdhw,cd->bhwc", sub, xw[k]).reshape(B, -1, CD)
        assert rel_err(out[k].cpu(), ref) < (1e-5 if mode == "fp32" else 1e-4), k


@pytest.mark.parametrize("mode,tol", MODES)
@pytest.mark.parametrize("C_", [32, 64, 256, 1024])
def test_ln_kernels(eng_factory, mode, tol, C_):
    from founddiff_amd import _lib as L
    e = eng_factory(mode)
    torch.manual_seed(3)
    B, hw = 2, 37
    x = rq(torch.randn(B, hw, C_) * 2 + 0.5, mode)
    g, b = torch.randn(C_), torch.randn(C_)
    mod = torch.randn(B, 3 * C_)
    sh, sc = mod[:, :C_], mod[:, C_:2 * C_]
    ref = F.layer_norm(x, (C_,), g, b, 1e-5) * (1 + sc[:, None]) + sh[:, None]
    xd, out = x.to("cuda", e.tdt), torch.empty(B, hw, C_, device="cuda", dtype=e.tdt)
    md, gd, bd = mod.cuda(), g.cuda(), b.cuda()     # keep device tensors alive across the launches
    L.call("fd_ln_modulate", e.dt, xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), 1e-5, md.data_ptr(),
           md.data_ptr() + 4 * C_, 3 * C_, out.data_ptr(), B, hw, C_, e.stream)
    torch.cuda.synchronize()
    assert rel_err(out.float().cpu(), ref) < tol
    ref2 = F.layer_norm(x, (C_,), None, None, 1e-6) * (1 + sc[:, None]) + sh[:, None]
    L.call("fd_ln_modulate", e.dt, xd.data_ptr(), None, None, 1e-6, md.data_ptr(), md.data_ptr() + 4 * C_, 3 * C_,
           out.data_ptr(), B, hw, C_, e.stream)
    torch.cuda.synchronize()
    assert rel_err(out.float().cpu(), ref2) < tol
    z = rq(torch.randn(B, hw, 2 * C_), mode)
    loc = torch.randn(B, C_ + 5)
    ref3 = F.layer_norm(x, (C_,), g, b, 1e-5) * z[..., C_:] + loc[:, None, 5:]
    ld = loc.cuda()
    zd = z.to("cuda", e.tdt)
    L.call("fd_ln_gate", e.dt, xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), 1e-5, zd.data_ptr(), 2 * C_,
           C_, ld.data_ptr() + 20, C_ + 5, out.data_ptr(), B, hw, C_, e.stream)
    torch.cuda.synchronize()
    assert rel_err(out.float().cpu(), ref3) < tol


@pytest.mark.parametrize("mode,tol", MODES)
def test_dwconv_avgpool_gn(eng_factory, mode, tol):
    from founddiff_amd import _lib as L
    e = eng_factory(mode)
    torch.manual_seed(4)
    B, Cc, H, W = 2, 48, 9, 14
    x = rq(torch.randn(B, Cc, H, W), mode)
    w, b = torch.randn(Cc, 1, 3, 3) / 3, torch.randn(Cc)
    ref = F.silu(F.conv2d(x, w, b, padding=1, groups=Cc))
    out = torch.empty(B, H, W, Cc, device="cuda", dtype=e.tdt)
    wd, bd, xd = w.reshape(Cc, 9).t().contiguous().cuda(), b.cuda(), nhwc(x, e.tdt)
    L.call("fd_dwconv3x3", e.dt, xd.data_ptr(), Cc, 0, wd.data_ptr(), bd.data_ptr(), 1,
           out.data_ptr(), Cc, 0, B, H, W, Cc, e.stream)
    torch.cuda.synchronize()
    assert rel_err(nchw(out), ref) < tol
    # several tiles / both row halves / channel blocks, strided channel window in and out, no SiLU
    Cb, Hb, Wb = 128, 40, 36
    xb = rq(torch.randn(B, Cb + 16, Hb, Wb), mode)
    wb, bb_ = torch.randn(Cb, 1, 3, 3) / 3, torch.randn(Cb)
    refb = F.conv2d(xb[:, 8:8 + Cb], wb, bb_, padding=1, groups=Cb)
    outb = torch.zeros(B, Hb, Wb, Cb + 8, device="cuda", dtype=e.tdt)
    wbd, bbd_, xbd = wb.reshape(Cb, 9).t().contiguous().cuda(), bb_.cuda(), nhwc(xb, e.tdt)
    L.call("fd_dwconv3x3", e.dt, xbd.data_ptr(), Cb + 16, 8, wbd.data_ptr(), bbd_.data_ptr(), 0,
           outb.data_ptr(), Cb + 8, 8, B, Hb, Wb, Cb, e.stream)
    torch.cuda.synchronize()
    assert rel_err(nchw(outb[..., 8:]), refb) < tol
    assert float(outb[..., :8].float().abs().max()) == 0.0
    x2 = rq(torch.randn(B, 16, 8, 12), mode)
    o2 = torch.empty(B, 4, 6, 16, device="cuda", dtype=e.tdt)
    x2d = nhwc(x2, e.tdt)
    L.call("fd_avgpool", e.dt, x2d.data_ptr(), o2.data_ptr(), B, 8, 12, 16, 2, e.stream)
    torch.cuda.synchronize()
    assert rel_err(nchw(o2), F.avg_pool2d(x2, 2)) < tol
    # GroupNorm + SiLU (+ residual) from mean/rstd
    h = rq(torch.randn(B, 32, 6, 5) * 3 + 1, mode)
    res = rq(torch.randn(B, 32, 6, 5), mode)
    g, bb = torch.randn(32), torch.randn(32)
    ref = F.silu(F.group_norm(h, 8, g, bb, 1e-5)) + res
    hv = h.reshape(B, 8, -1)
    mr = torch.stack([hv.mean(-1), torch.rsqrt(hv.var(-1, unbiased=False) + 1e-5)], -1).contiguous().cuda()
    o3 = torch.empty(B, 6, 5, 32, device="cuda", dtype=e.tdt)
    hd, gd, bbd, rd = nhwc(h, e.tdt), g.cuda(), bb.cuda(), nhwc(res, e.tdt)
    L.call("fd_gn_silu_apply", e.dt, hd.data_ptr(), mr.data_ptr(), gd.data_ptr(),
           bbd.data_ptr(), rd.data_ptr(), o3.data_ptr(), B, 30, 32, 8, e.stream)
    torch.cuda.synchronize()
    assert rel_err(nchw(o3), ref) < tol


# odd H and / or W: the reference's pad-to-even / crop (src/emamba2.py:191-199, 253-260) as index arithmetic
ODD_SHAPES = [(64, 4, 4, 15, 24), (64, 8, 2, 9, 7), (128, 32, 8, 13, 11), (128, 4, 4, 16, 37), (256, 16, 16, 63, 65)]


@pytest.mark.parametrize("mode,tol", MODES)
@pytest.mark.parametrize("cfg", [(64, 4, 4, 16, 24), (64, 8, 2, 8, 8), (128, 32, 8, 12, 10), (256, 16, 16, 64, 64)] + BLOCK_SHAPES + ODD_SHAPES)
def test_selective_scan(eng_factory, mode, tol, cfg):
    """HIP chunked scan (fused gather/dt_proj/softplus/merge) vs the sequential CPU oracle."""
    from founddiff_amd import _lib as L
    from oracle import nets
    e = eng_factory(mode)
    D, N, R, H, W = cfg
    torch.manual_seed(5)
    B, CD = 2, R + 2 * N
    H2, W2 = (H + 1) // 2, (W + 1) // 2
    Lq = H2 * W2
    xc = rq(torch.randn(B, D, H, W) * 0.5, mode)
    xdbl = torch.randn(4, B, Lq, CD)
    dtw = (torch.rand(4, D, R) * 2 - 1) * R ** -0.5
    dtb = torch.randn(4, D) * 0.5 - 3
    A = -torch.exp(torch.log(torch.arange(1, N + 1).float())[None].repeat(4 * D, 1) + 0.1 * torch.randn(4 * D, N))
    Ds = 1 + 0.1 * torch.randn(4 * D)
    # oracle on the explicitly gathered tensors
    ref, _ = scan_reference(xc, dtw, dtb, A, Ds, N, R, xdbl=xdbl, scan_fn=nets.selective_scan)
    nws = L.lib().fd_scan_ws_floats(B, H, W, D, N)
    ws = torch.empty(nws, device="cuda")
    y = torch.empty(B, H, W, D, device="cuda", dtype=e.tdt)
    t = [v.contiguous().cuda() for v in (xdbl, dtw, dtb, A, Ds)]
    xcd = nhwc(xc, e.tdt)
    L.call("fd_selective_scan", e.dt, xcd.data_ptr(), t[0].data_ptr(), t[1].data_ptr(),
           t[2].data_ptr(), t[3].data_ptr(), t[4].data_ptr(), y.data_ptr(), ws.data_ptr(), B, H, W, D, N, R, e.stream)
    torch.cuda.synchronize()
    gate2x(f"selective_scan[{'-'.join(map(str, cfg))}-{mode}]", rel_err(nchw(y), ref), 1e-4 if mode == "fp32" else 1e-2)


def _scan_inputs(b, KD, K, N, L, seed):
    g = torch.Generator().manual_seed(seed)
    u = torch.randn(b, KD, L, generator=g) * 0.5
    delta = torch.randn(b, KD, L, generator=g) * 0.5 - 2
    A = -torch.exp(torch.log(torch.arange(1, N + 1).float())[None].repeat(KD, 1) + 0.1 * torch.randn(KD, N, generator=g))
    Bm, Cm = torch.randn(b, K, N, L, generator=g), torch.randn(b, K, N, L, generator=g)
    D = 1 + 0.1 * torch.randn(KD, generator=g)
    bias = torch.randn(KD, generator=g) * 0.3
    return u, delta, A, Bm, Cm, D, bias


@pytest.mark.parametrize("cfg", [(d, n, 4 * d, 4, 200) for d, n, r, h, w in BLOCK_SHAPES] + [(64, 4, 128, 1, 37), (96, 6, 96, 2, 1029)])
def test_selective_scan_reference_signature(cfg):
    """selective_scan_cuda_core.fwd drop-in (include/founddiff_hip.h: fd_selective_scan_fwd_f32) in the reference's
    own operand layout (src/emamba2.py:124-154) against the sequential CPU oracle: the (d_inner, d_state) of every
    block with K = 4 groups, plus ragged lengths (L % 4 != 0, L > one 1024-position tile) and other group counts."""
    from founddiff_amd import selective_scan_cuda_core as ssc
    from oracle import nets
    D_, N, KD, K, Ln = cfg
    u, delta, A, Bm, Cm, D, bias = _scan_inputs(2, KD, K, N, Ln, seed=D_ + N)
    ref = nets.selective_scan(u, delta, A, Bm, Cm, D, bias, softplus=True)
    out, x = ssc.fwd(u.cuda(), delta.cuda(), A.cuda(), Bm.cuda(), Cm.cuda(), D.cuda(), bias.cuda(), True, 1)
    torch.cuda.synchronize()
    assert out.shape == u.shape and x.shape == (2, KD, N)
    assert rel_err(out.cpu(), ref) < 1e-5
    # no softplus, no D, no bias, 3-D B/C (single group), nrows = 2
    ref2 = nets.selective_scan(u, delta.abs() * 0.1, A, Bm[:, :1], Cm[:, :1], torch.zeros(KD), torch.zeros(KD), softplus=False)
    out2, _ = ssc.fwd(u.cuda(), (delta.abs() * 0.1).cuda(), A.cuda(), Bm[:, 0].contiguous().cuda(), Cm[:, 0].contiguous().cuda(),
                      None, None, False, 2)
    assert rel_err(out2.cpu(), ref2) < 1e-5
    # x = state after the last position: one more step from it reproduces the oracle on the extended sequence
    with pytest.raises(RuntimeError):
        ssc.fwd(u.cuda(), delta.cuda(), A.cuda(), Bm.cuda(), Cm.cuda(), D.cuda(), bias.cuda(), True, 5)      # nrows assert
    with pytest.raises(RuntimeError):
        ssc.fwd(u.cuda().double(), delta.cuda(), A.cuda(), Bm.cuda(), Cm.cuda(), D.cuda(), bias.cuda(), True, 1)


def test_selective_scan_long_sequence_vs_fp64():
    """L = 65 536 (one direction of a 512x512 image) against an fp64 sequential scan -- both native
    entry points: the reference-layout op and the engine's fused NHWC scan (fp32 mode)."""
    from founddiff_amd import _lib as L, selective_scan_cuda_core as ssc
    from oracle import nets
    N, R, D_, H, W = 4, 4, 64, 512, 512
    Lq = (H // 2) * (W // 2)
    assert Lq == 65536
    u, delta, A, Bm, Cm, D, bias = _scan_inputs(1, 4 * D_, 4, N, Lq, seed=11)
    ref = nets.selective_scan_f64(u, delta, A, Bm, Cm, D, bias)
    out, x = ssc.fwd(u.cuda(), delta.cuda(), A.cuda(), Bm.cuda(), Cm.cuda(), D.cuda(), bias.cuda(), True, 1)
    assert float((out.cpu().double() - ref).abs().max() / ref.abs().max()) < 2e-6
    # fused form: same recurrence through the gather / dt_proj / merge index maps
    torch.manual_seed(12)
    xc = torch.randn(1, D_, H, W) * 0.5
    xdbl = torch.randn(4, 1, Lq, R + 2 * N)
    dtw = (torch.rand(4, D_, R) * 2 - 1) * R ** -0.5
    dtb = torch.randn(4, D_) * 0.5 - 3
    A4 = -torch.exp(torch.log(torch.arange(1, N + 1).float())[None].repeat(4 * D_, 1) + 0.1 * torch.randn(4 * D_, N))
    Ds = 1 + 0.1 * torch.randn(4 * D_)
    xs = nets.efficient_scan(xc)
    xd = xdbl.permute(1, 0, 2, 3).reshape(1, 4, H // 2, W // 2, R + 2 * N)
    xd_scan = torch.stack([xd[:, 0].reshape(1, Lq, -1), xd[:, 1].transpose(1, 2).reshape(1, Lq, -1),
                           xd[:, 2].reshape(1, Lq, -1), xd[:, 3].transpose(1, 2).reshape(1, Lq, -1)], 1)
    dts = torch.einsum("bklr,kdr->bkdl", xd_scan[..., :R], dtw)
    Bs = xd_scan[..., R:R + N].permute(0, 1, 3, 2).contiguous()
    Cs = xd_scan[..., R + N:].permute(0, 1, 3, 2).contiguous()
    ys = nets.selective_scan_f64(xs.reshape(1, 4 * D_, Lq), dts.reshape(1, 4 * D_, Lq), A4, Bs, Cs, Ds, dtb.reshape(-1))
    ref = nets.efficient_merge(ys.view(1, 4, D_, Lq), H, W).view(1, D_, H, W)
    ws = torch.empty(L.lib().fd_scan_ws_floats(1, H, W, D_, N), device="cuda")
    y = torch.empty(1, H, W, D_, device="cuda")
    t = [v.contiguous().cuda() for v in (xdbl, dtw, dtb, A4, Ds)]
    xcd = nhwc(xc, torch.float32)
    L.call("fd_selective_scan", L.FD_F32, xcd.data_ptr(), t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(),
           t[4].data_ptr(), y.data_ptr(), ws.data_ptr(), 1, H, W, D_, N, R, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert float((nchw(y).double() - ref).abs().max() / ref.abs().max()) < 1e-5


@pytest.mark.parametrize("mode,tol", MODES)
def test_channel_attention(eng_factory, mode, tol):
    from founddiff_amd import _lib as L
    from oracle import nets
    e = eng_factory(mode)
    torch.manual_seed(6)
    B, Cc, H, W = 2, 64, 40, 30          # hw = 1200 -> 2 pixel blocks, ragged tail
    qkv = rq(torch.randn(B, 3 * Cc, H, W), mode)
    temp = 1 + 0.3 * torch.randn(2)
    wp = torch.randn(Cc, Cc) / 8
    res = rq(torch.randn(B, Cc, H, W), mode)
    gate = torch.randn(B, Cc)
    q, k, v = qkv.chunk(3, 1)
    qh = F.normalize(q.reshape(B, 2, 32, -1), dim=-1)
    kh = F.normalize(k.reshape(B, 2, 32, -1), dim=-1)
    attn = ((qh @ kh.transpose(-2, -1)) * temp[None, :, None, None]).softmax(-1)
    o = (attn @ v.reshape(B, 2, 32, -1)).reshape(B, Cc, H, W)
    ref = res + gate[:, :, None, None] * F.conv2d(o, wp[:, :, None, None])
    qd = nhwc(qkv, e.tdt)
    nblk = L.lib().fd_chan_attn_nblk(H * W)
    part = torch.empty(B, 2, nblk, 1024 + 64, device="cuda")
    L.call("fd_chan_attn_gram", e.dt, qd.data_ptr(), B, H * W, Cc, part.data_ptr(), e.stream)
    weff = torch.empty(B, Cc, Cc, device="cuda", dtype=e.tdt)
    td, wpd = temp.cuda(), wp.cuda()
    L.call("fd_chan_attn_weff", e.dt, part.data_ptr(), nblk, td.data_ptr(), wpd.data_ptr(),
           weff.data_ptr(), B, Cc, e.stream)
    out = torch.empty(B, H, W, Cc, device="cuda", dtype=e.tdt)
    e.conv(None, qd, B, H, W, out, c0=Cc, ld0=3 * Cc, off0=2 * Cc, weight=weff, w_batch_stride=Cc * Cc, bias=None,
           Cout=Cc, KH=1, KW=1, epi=L.EPI_GATE_RES, res=nhwc(res, e.tdt), gate=gate.cuda(), gate_ld=Cc)
    torch.cuda.synchronize()
    assert rel_err(nchw(out), ref) < tol


def test_small_fp32_ops(eng_factory):
    from founddiff_amd import _lib as L
    from oracle import nets
    e = eng_factory("fp32")
    torch.manual_seed(7)
    x, w, b = torch.randn(3, 200), torch.randn(77, 200) / 14, torch.randn(77)
    for act, fn in ((0, lambda v: v), (1, F.silu), (2, F.gelu), (3, F.relu)):
        out = torch.empty(3, 77, device="cuda")
        e.linear(x.cuda(), w.cuda(), b.cuda(), out, act)
        assert rel_err(out.cpu(), fn(F.linear(x, w, b))) < 1e-5
    out = torch.empty(3, 77, device="cuda")
    e.linear(x.cuda(), w.cuda(), None, out, 0, pre_silu=True)
    assert rel_err(out.cpu(), F.linear(F.silu(x), w)) < 1e-5
    t = torch.tensor([998.5, 3.25, 0.0])
    emb = torch.empty(3, 64, device="cuda")
    td = t.cuda()
    L.call("fd_sinusoidal", td.data_ptr(), emb.data_ptr(), 3, 64, e.stream)
    assert rel_err(emb.cpu(), nets.sinusoidal_emb(t, 64)) < 2e-4     # sin/cos of ~1e3 rad in fp32
    p = torch.rand(77)
    o = torch.empty(3, 77, device="cuda")
    pd = p.cuda()
    L.call("fd_softmax_mul", out.data_ptr(), pd.data_ptr(), o.data_ptr(), 3, 77, e.stream)
    assert rel_err(o.cpu(), torch.softmax(out.cpu(), 1) * p) < 1e-5
    L.call("fd_l2norm_rows", out.data_ptr(), o.data_ptr(), 3, 77, 1e-12, e.stream)
    assert rel_err(o.cpu(), F.normalize(out.cpu(), dim=1)) < 1e-5
    # attention pool core
    B, T, Cf, heads = 2, 17, 128, 2
    qkv = torch.randn(B, T, 3 * Cf)
    q = qkv[:, 0, :Cf].reshape(B, heads, 1, 64) * 64 ** -0.5
    k = qkv[:, :, Cf:2 * Cf].reshape(B, T, heads, 64).permute(0, 2, 1, 3)
    v = qkv[:, :, 2 * Cf:].reshape(B, T, heads, 64).permute(0, 2, 1, 3)
    ref = ((q @ k.transpose(-2, -1)).softmax(-1) @ v).reshape(B, Cf)
    qd = qkv.cuda()
    po = torch.empty(B, Cf, device="cuda")
    L.call("fd_attnpool_core", qd.data_ptr(), T * 3 * Cf, qd.data_ptr(), 3 * Cf, Cf, 2 * Cf, po.data_ptr(), B, T, Cf,
           heads, e.stream)
    assert rel_err(po.cpu(), ref) < 1e-5


def test_row_gemm_fused_prologues(eng_factory):
    """bf16 streaming row-GEMM (1x1 convs of the high-resolution levels) incl. fused LayerNorm
    prologues, two-source A operand, per-batch weights and every epilogue it serves."""
    from founddiff_amd import _lib as L
    from founddiff_amd.engine import ConvW
    e = eng_factory("bf16")
    torch.manual_seed(11)
    B, H, W = 2, 128, 256                       # 32768 pixels per image: row-GEMM territory
    hw = H * W
    bf = lambda t: t.to(HB.t).float()

    def run(cw, x, out, **kw):
        assert e.conv(cw, x, B, H, W, out, probe=True, **kw), "expected the row-GEMM path"
        e.conv(cw, x, B, H, W, out, **kw)
        torch.cuda.synchronize()
        return out.float().cpu()

    # (1) in_proj: LN + adaLN modulate prologue, SiLU on the z half
    x = bf(torch.randn(B, hw, 64) * 1.5 + 0.3)
    w = bf(torch.randn(256, 64) / 8)
    g, b_ = torch.randn(64), torch.randn(64)
    mod = torch.randn(B, 6 * 64) * 0.5
    xd, md, gd, bd = x.cuda().to(HB.t), mod.cuda(), g.cuda(), b_.cuda()
    xm = F.layer_norm(x, (64,), g, b_, 1e-5) * (1 + mod[:, None, 64:128]) + mod[:, None, 0:64]
    ref = F.linear(bf(xm), w)
    ref[..., 128:] = F.silu(ref[..., 128:])
    out = torch.empty(B, H, W, 256, device="cuda", dtype=HB.t)
    got = run(ConvW(w, None, e.dev, e.tdt), xd, out, epi=L.EPI_SILU_SPLIT, split=128, prologue=L.PRO_LN_MOD,
              ln_gamma=gd, ln_beta=bd, ln_eps=1e-5, ln_shift=C.c_void_p(md.data_ptr()),
              ln_scale=C.c_void_p(md.data_ptr() + 64 * 4), ln_ld=6 * 64)
    assert rel_err(got.reshape(B, hw, 256), ref) < 1.5e-2
    # (2) out_proj: out_norm(y) * z + local prologue, gated residual epilogue
    y = bf(torch.randn(B, hw, 128) * 2)
    xz = bf(torch.randn(B, hw, 256))
    loc = torch.randn(B, 128)
    w2 = bf(torch.randn(64, 128) / 11)
    g2, b2 = torch.randn(128), torch.randn(128)
    res = bf(torch.randn(B, hw, 64))
    yz = F.layer_norm(y, (128,), g2, b2, 1e-5) * xz[..., 128:] + loc[:, None]
    ref = res + mod[:, None, 128:192] * F.linear(bf(yz), w2)
    yd, xzd, locd, g2d, b2d, resd = (y.cuda().to(HB.t), xz.cuda().to(HB.t), loc.cuda(),
                                     g2.cuda(), b2.cuda(), res.cuda().to(HB.t))
    out = torch.empty(B, H, W, 64, device="cuda", dtype=HB.t)
    got = run(ConvW(w2, None, e.dev, e.tdt), yd, out, epi=L.EPI_GATE_RES, res=resd,
              gate=C.c_void_p(md.data_ptr() + 128 * 4), gate_ld=6 * 64, prologue=L.PRO_LN_GATE, ln_gamma=g2d,
              ln_beta=b2d, ln_eps=1e-5, ln_shift=locd, ln_ld=128, ln_z=xzd, ln_ldz=256, ln_offz=128)
    assert rel_err(got.reshape(B, hw, 64), ref) < 1.5e-2
    # (2b) the same out_proj with the z gate RECOMPUTED from the residual operand (PRO_LN_GATE_ZRE): z = SiLU(W_z .
    # LNmod(res)) rounded to bf16 as the fused in_proj stores it; against torch and against (2)'s kernel fed that z
    wz = bf(torch.randn(128, 64) / 8)
    xm2 = F.layer_norm(res, (64,), g, b_, 1e-5) * (1 + mod[:, None, 64:128]) + mod[:, None, 0:64]
    zt = bf(F.silu(F.linear(bf(xm2), wz)))
    ref = res + mod[:, None, 128:192] * F.linear(bf((F.layer_norm(y, (128,), g2, b2, 1e-5) * zt + loc[:, None])), w2)
    wzd = wz.cuda().to(HB.t)
    kwz = dict(epi=L.EPI_GATE_RES, res=resd, gate=C.c_void_p(md.data_ptr() + 128 * 4), gate_ld=6 * 64, ln_gamma=g2d,
               ln_beta=b2d, ln_eps=1e-5, ln_shift=locd, ln_ld=128)
    out = torch.empty(B, H, W, 64, device="cuda", dtype=HB.t)
    got = run(ConvW(w2, None, e.dev, e.tdt), yd, out, prologue=L.PRO_LN_GATE_ZRE,
              zre=dict(w=wzd, gamma=gd, beta=bd, shift=C.c_void_p(md.data_ptr()), scale=C.c_void_p(md.data_ptr() + 64 * 4),
                       ld=6 * 64, eps=1e-5), **kwz)
    assert rel_err(got.reshape(B, hw, 64), ref) < 1.5e-2
    ztd = torch.zeros(B, hw, 256, dtype=HB.t, device="cuda")
    ztd[..., 128:] = zt.cuda().to(HB.t)
    out2 = torch.empty(B, H, W, 64, device="cuda", dtype=HB.t)
    stored = run(ConvW(w2, None, e.dev, e.tdt), yd, out2, prologue=L.PRO_LN_GATE, ln_z=ztd, ln_ldz=256, ln_offz=128, **kwz)
    assert rel_err(got, stored) < 4e-3            # same operands up to bf16 flips of LNmod(res) / z at rounding ties
    # a ragged pixel count (H * W not a multiple of 16) and unaffine norm1
    Hr, Wr = 127, 255
    hwr = Hr * Wr
    outr = torch.empty(B, Hr, Wr, 64, device="cuda", dtype=HB.t)
    yr_, rr_ = yd.reshape(B, hw, 128)[:, :hwr].contiguous(), resd.reshape(B, hw, 64)[:, :hwr].contiguous()
    kwr = dict(kwz, res=rr_)
    assert e.conv(ConvW(w2, None, e.dev, e.tdt), yr_, B, Hr, Wr, outr, probe=True, prologue=L.PRO_LN_GATE_ZRE,
                  zre=dict(w=wzd, shift=C.c_void_p(md.data_ptr()), scale=C.c_void_p(md.data_ptr() + 64 * 4), ld=6 * 64, eps=1e-5), **kwr)
    e.conv(ConvW(w2, None, e.dev, e.tdt), yr_, B, Hr, Wr, outr, prologue=L.PRO_LN_GATE_ZRE,
           zre=dict(w=wzd, shift=C.c_void_p(md.data_ptr()), scale=C.c_void_p(md.data_ptr() + 64 * 4), ld=6 * 64, eps=1e-5), **kwr)
    torch.cuda.synchronize()
    xm3 = F.layer_norm(res[:, :hwr], (64,), None, None, 1e-5) * (1 + mod[:, None, 64:128]) + mod[:, None, 0:64]
    zt3 = bf(F.silu(F.linear(bf(xm3), wz)))
    ref3 = res[:, :hwr] + mod[:, None, 128:192] * F.linear(bf((F.layer_norm(y[:, :hwr], (128,), g2, b2, 1e-5) * zt3 + loc[:, None])), w2)
    assert rel_err(outr.float().cpu().reshape(B, hwr, 64), ref3) < 1.5e-2
    # the K = 256 instance (the C = 128 blocks: d_inner 256)
    y8, res8 = bf(torch.randn(B, hw, 256) * 2), bf(torch.randn(B, hw, 128))
    w8, wz8 = bf(torch.randn(128, 256) / 16), bf(torch.randn(256, 128) / 11)
    g8, b8, go8, bo8, loc8 = torch.randn(128), torch.randn(128), torch.randn(256), torch.randn(256), torch.randn(B, 256)
    mod8 = torch.randn(B, 6 * 128) * 0.5
    xm8 = F.layer_norm(res8, (128,), g8, b8, 1e-5) * (1 + mod8[:, None, 128:256]) + mod8[:, None, 0:128]
    zt8 = bf(F.silu(F.linear(bf(xm8), wz8)))
    ref8 = res8 + mod8[:, None, 256:384] * F.linear(bf((F.layer_norm(y8, (256,), go8, bo8, 1e-5) * zt8 + loc8[:, None])), w8)
    m8d = mod8.cuda()
    out8 = torch.empty(B, H, W, 128, device="cuda", dtype=HB.t)
    got8 = run(ConvW(w8, None, e.dev, e.tdt), y8.cuda().to(HB.t), out8, prologue=L.PRO_LN_GATE_ZRE,
               epi=L.EPI_GATE_RES, res=res8.cuda().to(HB.t), gate=C.c_void_p(m8d.data_ptr() + 256 * 4), gate_ld=6 * 128,
               ln_gamma=go8.cuda(), ln_beta=bo8.cuda(), ln_eps=1e-5, ln_shift=loc8.cuda(), ln_ld=256,
               zre=dict(w=wz8.cuda().to(HB.t), gamma=g8.cuda(), beta=b8.cuda(), shift=C.c_void_p(m8d.data_ptr()),
                        scale=C.c_void_p(m8d.data_ptr() + 128 * 4), ld=6 * 128, eps=1e-5))
    assert rel_err(got8.reshape(B, hw, 128), ref8) < 1.5e-2
    # (3) res_conv over a concat (128 + 64 -> 128) fused with GroupNorm+SiLU of the 3x3 output
    a, c = bf(torch.randn(B, hw, 128)), bf(torch.randn(B, hw, 64))
    w3, bias3 = bf(torch.randn(128, 192) / 14), torch.randn(128)
    h = bf(torch.randn(B, hw, 128) * 2 + 1)
    gg, gb = torch.randn(128), torch.randn(128)
    hv = h.reshape(B, hw, 8, 16).permute(0, 2, 1, 3).reshape(B, 8, -1)
    mr = torch.stack([hv.mean(-1), torch.rsqrt(hv.var(-1, unbiased=False) + 1e-5)], -1).contiguous()
    gn = F.group_norm(h.permute(0, 2, 1), 8, gg, gb, 1e-5).permute(0, 2, 1)
    ref = F.linear(torch.cat((a, c), -1), w3, bias3) + F.silu(gn)
    ad, cd, hd, mrd, ggd, gbd = (a.cuda().to(HB.t), c.cuda().to(HB.t),
                                 h.cuda().to(HB.t), mr.cuda(), gg.cuda(), gb.cuda())
    out = torch.empty(B, H, W, 128, device="cuda", dtype=HB.t)
    got = run(ConvW(w3, bias3, e.dev, e.tdt), ad, out, c0=128, in1=cd, c1=64, epi=L.EPI_GNSILU_ADD, h=hd, gn=mrd,
              gamma=ggd, beta=gbd, groups=8)
    assert rel_err(got.reshape(B, hw, 128), ref) < 1.5e-2
    # (4) per-batch weights on a channel slice (attn@v folded with project_out)
    big = bf(torch.randn(B, hw, 192))
    wb = bf(torch.randn(B, 64, 64) / 8)
    ref = res + mod[:, None, 320:384] * torch.einsum("bmk,bnk->bmn", big[..., 128:], wb)
    bigd, wbd = big.cuda().to(HB.t), wb.cuda().to(HB.t)
    out = torch.empty(B, H, W, 64, device="cuda", dtype=HB.t)
    got = run(None, bigd, out, c0=64, ld0=192, off0=128, weight=wbd, w_batch_stride=64 * 64, bias=None, Cout=64,
              KH=1, KW=1, epi=L.EPI_GATE_RES, res=resd, gate=C.c_void_p(md.data_ptr() + 320 * 4), gate_ld=6 * 64)
    assert rel_err(got.reshape(B, hw, 64), ref) < 1.5e-2
    # (5) wide Cout: the weight image (512 x 256 B = 128 KiB) leaves one workgroup per CU -> 12-wave
    # workgroups; LN + modulate prologue over K = 128, SiLU on the upper half
    x5 = bf(torch.randn(B, hw, 128) * 1.5 - 0.2)
    w5 = bf(torch.randn(512, 128) / 11)
    g5, b5 = torch.randn(128), torch.randn(128)
    mod5 = torch.randn(B, 6 * 128) * 0.5
    x5d, m5d, g5d, b5d = x5.cuda().to(HB.t), mod5.cuda(), g5.cuda(), b5.cuda()
    xm = F.layer_norm(x5, (128,), g5, b5, 1e-5) * (1 + mod5[:, None, 128:256]) + mod5[:, None, 0:128]
    ref = F.linear(bf(xm), w5)
    ref[..., 256:] = F.silu(ref[..., 256:])
    out = torch.empty(B, H, W, 512, device="cuda", dtype=HB.t)
    got = run(ConvW(w5, None, e.dev, e.tdt), x5d, out, epi=L.EPI_SILU_SPLIT, split=256, prologue=L.PRO_LN_MOD,
              ln_gamma=g5d, ln_beta=b5d, ln_eps=1e-5, ln_shift=C.c_void_p(m5d.data_ptr()),
              ln_scale=C.c_void_p(m5d.data_ptr() + 128 * 4), ln_ld=6 * 128)
    assert rel_err(got.reshape(B, hw, 512), ref) < 1.5e-2
    # (6) K = 256 -> 128 (64 KiB of weights: two 8-wave workgroups per CU), residual + ReLU epilogue
    x6 = bf(torch.randn(B, hw, 256))
    w6, bias6 = bf(torch.randn(128, 256) / 16), torch.randn(128)
    res6 = bf(torch.randn(B, hw, 128))
    ref = F.relu(F.linear(x6, w6, bias6) + res6)
    x6d, r6d = x6.cuda().to(HB.t), res6.cuda().to(HB.t)
    out = torch.empty(B, H, W, 128, device="cuda", dtype=HB.t)
    got = run(ConvW(w6, bias6, e.dev, e.tdt), x6d, out, epi=L.EPI_RES_RELU, res=r6d)
    assert rel_err(got.reshape(B, hw, 128), ref) < 1.5e-2


@pytest.mark.parametrize("cfg", [
    dict(c0=64, c1=0, cout=64, hw=(64, 64), up=False, relu=False),      # <64, 16>: 16x16 tile, 64x64 wave tiles
    dict(c0=64, c1=64, cout=192, hw=(72, 80), up=False, relu=False),    # <128, 8>: two sources, ragged last N tile
    dict(c0=64, c1=0, cout=40, hw=(72, 64), up=True, relu=True),        # <64, 8>: OH % 16 != 0, x2 upsample, ReLU
])
def test_conv3x3_halo(eng_factory, cfg):
    """Halo-tiled 3x3 implicit GEMM (bf16): every tile variant, with the GroupNorm partial sums."""
    from founddiff_amd import _lib as L
    from founddiff_amd.engine import ConvW
    e = eng_factory("bf16")
    torch.manual_seed(21)
    B = 2
    OH, OW = cfg["hw"]
    H, W = (OH // 2, OW // 2) if cfg["up"] else (OH, OW)
    cin = cfg["c0"] + cfg["c1"]
    x = rq(torch.randn(B, cin, H, W), "bf16")
    w = rq(torch.randn(cfg["cout"], cin, 3, 3) / (3 * cin ** 0.5), "bf16")
    bias = torch.randn(cfg["cout"])
    xin = F.interpolate(x, scale_factor=2, mode="nearest") if cfg["up"] else x
    ref = F.conv2d(xin, w, bias, padding=1)
    if cfg["relu"]:
        ref = F.relu(ref)
    cw = ConvW(w, bias, e.dev, e.tdt)
    out = torch.empty(B, OH, OW, cfg["cout"], device="cuda", dtype=e.tdt)
    part = torch.full((B, L.lib().fd_conv_mtiles(OH, OW), cfg["cout"], 2), 7.0, device="cuda")   # must be overwritten
    kw = dict(c0=cfg["c0"], stats=part, upsample=cfg["up"], epi=L.EPI_RELU if cfg["relu"] else L.EPI_NONE)
    xa = nhwc(x[:, :cfg["c0"]], e.tdt)
    if cfg["c1"]:
        kw.update(in1=nhwc(x[:, cfg["c0"]:], e.tdt), c1=cfg["c1"])
    assert e.conv(cw, xa, B, H, W, out, probe="kid", **kw) == 11, "expected the halo-tiled kernel"
    e.conv(cw, xa, B, H, W, out, **kw)
    torch.cuda.synchronize()
    assert rel_err(nchw(out), ref) < 1.2e-2
    s = part.sum(1).cpu()
    assert rel_err(s[..., 0], ref.sum((2, 3))) < 5e-3
    assert rel_err(s[..., 1], (ref ** 2).sum((2, 3))) < 5e-3
    # the weight ring's s_waitcnt bookkeeping is manual: a tile read before its DMA landed would show up as
    # run-to-run differences -- 16 more launches must reproduce the first one bit for bit
    first, first_part = out.clone(), part.clone()
    for _ in range(16):
        out.zero_()
        e.conv(cw, xa, B, H, W, out, **kw)
        torch.cuda.synchronize()
        assert torch.equal(out, first) and torch.equal(part, first_part)


@pytest.mark.parametrize("hw", [(256, 512), (272, 512)])
def test_conv3x3_weights_in_registers(eng_factory, hw):
    """3x3 64 -> 64 with the weight matrix resident in registers (fd_conv3x3_rw.hip, kernel id 13; the first convolution of the
    64-channel ResnetBlocks at >= 131072 pixels) against torch and against the halo-tiled kernel (FD_NO_CONV3_RW is read once
    per process, so the halo kernel is reached through a two-source split of the same channels), with the GroupNorm partial
    sums; the second size leaves the last workgroup one tile of three."""
    from founddiff_amd import _lib as L
    from founddiff_amd.engine import ConvW
    e = eng_factory("bf16")
    torch.manual_seed(23)
    B, (H, W) = 2, hw
    x = rq(torch.randn(B, 64, H, W), "bf16")
    w = rq(torch.randn(64, 64, 3, 3) / 24, "bf16")
    bias = torch.randn(64)
    ref = F.conv2d(x, w, bias, padding=1)
    cw = ConvW(w, bias, e.dev, e.tdt)
    xa = nhwc(x, e.tdt)
    out = torch.empty(B, H, W, 64, device="cuda", dtype=e.tdt)
    part = torch.full((B, L.lib().fd_conv_mtiles(H, W), 64, 2), 7.0, device="cuda")       # must be overwritten
    kw = dict(c0=64, stats=part)
    assert e.conv(cw, xa, B, H, W, out, probe="kid", **kw) == 13
    e.conv(cw, xa, B, H, W, out, **kw)
    torch.cuda.synchronize()
    assert rel_err(nchw(out), ref) < 1.2e-2
    s = part.sum(1).cpu()
    assert rel_err(s[..., 0], ref.sum((2, 3))) < 5e-3 and rel_err(s[..., 1], (ref ** 2).sum((2, 3))) < 5e-3
    # the halo-tiled kernel on the same operands (input handed over as two 32-channel sources is not eligible for id 13 -- c0 must
    # be 64 -- nor for the halo kernel's 64-channel slabs; use the plain kernel through a 128-channel zero-extended input instead)
    x2 = torch.zeros(B, H, W, 128, device="cuda", dtype=e.tdt)
    x2[..., :64] = xa
    w2 = torch.zeros(64, 128, 3, 3)
    w2[:, :64] = w
    out2 = torch.empty_like(out)
    cw2 = ConvW(w2, bias, e.dev, e.tdt)
    assert e.conv(cw2, x2, B, H, W, out2, probe="kid", c0=128) == 11
    e.conv(cw2, x2, B, H, W, out2, c0=128)
    torch.cuda.synchronize()
    assert rel_err(out.float().cpu(), out2.float().cpu()) < 4e-3          # bf16 outputs of fp32 sums in two orders
    first, first_part = out.clone(), part.clone()
    for _ in range(4):
        out.zero_()
        e.conv(cw, xa, B, H, W, out, **kw)
        torch.cuda.synchronize()
        assert torch.equal(out, first) and torch.equal(part, first_part)


@pytest.mark.parametrize("cfg", [dict(cdw=128, cz=128, silu=1, bias=True, affine=True, hw=(128, 256)),     # SS2D in_proj + conv2d
                                 dict(cdw=192, cz=0, silu=0, bias=False, affine=False, hw=(256, 128)),    # qkv + qkv_dwconv
                                 dict(cdw=256, cz=256, silu=1, bias=True, affine=True, hw=(128, 256), cin=128),   # C = 128 in_proj
                                 dict(cdw=256, cz=256, silu=1, bias=True, affine=True, hw=(264, 144), cin=128)])  # 297 tiles (B = 2: one per workgroup; the
                                 # several-tiles walk and its ragged last workgroup: tests/test_gpu_pwdw_forms.py)
def test_pw_dw3x3_fused(eng_factory, cfg):
    """Fused LN+modulate -> 1x1 -> depthwise 3x3 (bf16) against the unfused fp32 composition; borders
    included (the depthwise conv zero-pads the 1x1 OUTPUT)."""
    from founddiff_amd import _lib as L
    from founddiff_amd.engine import DAEngine
    e = eng_factory("bf16")
    torch.manual_seed(31)
    B, (H, W), Cin = 2, cfg["hw"], cfg.get("cin", 64)
    cdw, cz = cfg["cdw"], cfg["cz"]
    bf = lambda t: t.to(HB.t).float()
    x = bf(torch.randn(B, H, W, Cin) * 1.3 + 0.2)
    g, be = (torch.randn(Cin), torch.randn(Cin)) if cfg["affine"] else (None, None)
    mod = torch.randn(B, 6 * Cin) * 0.5
    wpw = bf(torch.randn(cdw + cz, Cin) / Cin ** 0.5)
    wdw = torch.randn(cdw, 1, 3, 3) / 3
    bdw = torch.randn(cdw) if cfg["bias"] else None
    eps = 1e-5 if cfg["affine"] else 1e-6
    xn = F.layer_norm(x, (Cin,), g, be, eps) * (1 + mod[:, None, None, Cin:2 * Cin]) + mod[:, None, None, :Cin]
    t = bf(F.linear(bf(xn), wpw))                                    # 1x1 output, rounded where the kernel rounds
    ref_dw = F.conv2d(t[..., :cdw].permute(0, 3, 1, 2), bf(wdw), bdw, padding=1, groups=cdw)
    if cfg["silu"]:
        ref_dw = F.silu(ref_dw)
    assert L.lib().fd_pw_dw3x3_ok(L.FD_BF16, Cin, cdw, cz, H, W)
    xd, md = x.cuda().to(HB.t), mod.cuda()
    wpd = wpw.cuda().to(HB.t)
    wm = DAEngine._dw_masked(wdw.reshape(cdw, 9).t().contiguous().cuda())
    out_dw = torch.zeros(B, H, W, cdw + 8, device="cuda", dtype=HB.t)
    out_z = torch.zeros(B, H, W, 2 * cz + 8, device="cuda", dtype=HB.t)
    gd, bd = (g.cuda(), be.cuda()) if cfg["affine"] else (None, None)
    bdd = bdw.cuda() if bdw is not None else None
    ptr = lambda t_: None if t_ is None else t_.data_ptr()
    L.call("fd_pw_dw3x3", L.FD_BF16, xd.data_ptr(), Cin, 0, Cin, ptr(gd), ptr(bd), eps, md.data_ptr(),
           md.data_ptr() + Cin * 4, 6 * Cin, wpd.data_ptr(), cdw, wm.data_ptr(), ptr(bdd), cfg["silu"],
           out_dw.data_ptr(), cdw + 8, 8, cz, out_z.data_ptr(), 2 * cz + 8, cz, B, H, W, None)
    torch.cuda.synchronize()
    got = out_dw[..., 8:].float().cpu().permute(0, 3, 1, 2)
    assert rel_err(got, ref_dw) < 1.2e-2
    # border rows / columns separately: a wrong padding rule hides in the global norm
    assert rel_err(got[:, :, 0], ref_dw[:, :, 0]) < 1.5e-2 and rel_err(got[:, :, :, -1], ref_dw[:, :, :, -1]) < 1.5e-2
    assert float(out_dw[..., :8].float().abs().max()) == 0.0
    if cz:
        ref_z = F.silu(t[..., cdw:])
        assert rel_err(out_z[..., cz:2 * cz].float().cpu(), ref_z) < 1.2e-2
        assert float(out_z[..., :cz].float().abs().max()) == 0.0 and float(out_z[..., 2 * cz:].float().abs().max()) == 0.0


@pytest.mark.parametrize("hw", [(128, 256), (264, 144)])
def test_pw_dw3x3_gram(eng_factory, hw):
    """qkv -> qkv_dwconv -> L2 norms + q k^T in one kernel (fd_pw_dw3x3_gram, src/DADiff.py:266-276): the v it
    writes, and the reduced Gram / sums of squares, against (a) the unfused HIP pair fd_pw_dw3x3 + fd_chan_attn_gram
    on the same inputs (same bf16 rounding points: agreement to fp32 summation order) and (b) the fp32 composition.
    The second size has a tile count that is not a multiple of the tiles per workgroup (ragged last workgroup)."""
    from founddiff_amd import _lib as L
    from founddiff_amd.engine import DAEngine
    torch.manual_seed(33)
    B, (H, W), Cin = 2, hw, 64
    bf = lambda t: t.to(HB.t).float()
    x = bf(torch.randn(B, H, W, Cin) * 1.3 + 0.2)
    mod = torch.randn(B, 6 * Cin) * 0.5
    wpw = bf(torch.randn(192, Cin) / 8)
    wdw = torch.randn(192, 1, 3, 3) / 3
    assert L.lib().fd_pw_dw3x3_gram_ok(L.FD_BF16, Cin, H, W)
    xd, md = x.cuda().to(HB.t), mod.cuda()
    wpd = wpw.cuda().to(HB.t)
    wm = DAEngine._dw_masked(wdw.reshape(192, 9).t().contiguous().cuda())
    s = torch.cuda.current_stream().cuda_stream
    # unfused HIP pair
    qkv2 = torch.empty(B, H, W, 192, device="cuda", dtype=HB.t)
    L.call("fd_pw_dw3x3", L.FD_BF16, xd.data_ptr(), Cin, 0, Cin, None, None, 1e-6, md.data_ptr(), md.data_ptr() + Cin * 4,
           6 * Cin, wpd.data_ptr(), 192, wm.data_ptr(), None, 0, qkv2.data_ptr(), 192, 0, 0, None, 0, 0, B, H, W, s)
    nb0 = L.lib().fd_chan_attn_nblk(H * W)
    part0 = torch.empty(B, 2, nb0, 1088, device="cuda")
    L.call("fd_chan_attn_gram", L.FD_BF16, qkv2.data_ptr(), B, H * W, Cin, part0.data_ptr(), s)
    # fused
    nb1 = L.lib().fd_pw_dw3x3_gram_nblk(H, W)
    part1 = torch.full((B, 2, nb1, 1088), float("nan"), device="cuda")
    v = torch.zeros(B, H, W, 64 + 8, device="cuda", dtype=HB.t)
    L.call("fd_pw_dw3x3_gram", L.FD_BF16, xd.data_ptr(), Cin, 0, Cin, None, None, 1e-6, md.data_ptr(), md.data_ptr() + Cin * 4,
           6 * Cin, wpd.data_ptr(), wm.data_ptr(), v.data_ptr(), 64 + 8, 8, part1.data_ptr(), B, H, W, s)
    torch.cuda.synchronize()
    assert torch.equal(v[..., 8:], qkv2[..., 128:]) and float(v[..., :8].float().abs().max()) == 0.0
    g0, g1 = part0.double().sum(2).cpu(), part1.double().sum(2).cpu()
    assert bool(torch.isfinite(g1).all())
    # the unfused pair rounds q, k to bf16 on their way through HBM; fused they stay fp16 on chip (3 more bits): the
    # Gram entries (sums over all pixels of products with random signs) agree to ~1e-3 of the largest entry
    assert rel_err(g1[..., :1024], g0[..., :1024]) < 3e-3 and rel_err(g1[..., 1024:], g0[..., 1024:]) < 3e-3
    # fp32 composition (LayerNorm -> 1x1 -> depthwise in fp32 from the same bf16 inputs / weights): the fused kernel is the
    # CLOSER of the two
    xn = F.layer_norm(x, (Cin,), None, None, 1e-6) * (1 + mod[:, None, None, Cin:2 * Cin]) + mod[:, None, None, :Cin]
    t = F.linear(bf(xn), wpw)
    dwo = F.conv2d(t.permute(0, 3, 1, 2), wdw, None, padding=1, groups=192).permute(0, 2, 3, 1)
    q, k = dwo[..., :64].reshape(B, H * W, 2, 32), dwo[..., 64:128].reshape(B, H * W, 2, 32)
    gram = torch.einsum("bphi,bphj->bhij", q.double(), k.double()).reshape(B, 2, 1024)
    e_f, e_u = rel_err(g1[..., :1024], gram), rel_err(g0[..., :1024], gram)
    # (on the binary16 build the unfused pair -- fp32-accumulating depthwise, q / k rounded to nearest -- is the closer one by a
    #  factor of two: the fused kernel's depthwise accumulates its nine taps in fp16; both far inside the gate)
    assert e_f < 4e-3 and (HB.fp16 or e_f < 1.5 * e_u + 1e-4), (e_f, e_u)
    assert rel_err(g1[..., 1024:1056], (q.double() ** 2).sum(1)) < 4e-3 and rel_err(g1[..., 1056:], (k.double() ** 2).sum(1)) < 4e-3
    # deterministic
    part2 = torch.empty_like(part1)
    L.call("fd_pw_dw3x3_gram", L.FD_BF16, xd.data_ptr(), Cin, 0, Cin, None, None, 1e-6, md.data_ptr(), md.data_ptr() + Cin * 4,
           6 * Cin, wpd.data_ptr(), wm.data_ptr(), v.data_ptr(), 64 + 8, 8, part2.data_ptr(), B, H, W, s)
    torch.cuda.synchronize()
    assert torch.equal(part1, part2)
    # q, k only (out_v = NULL): the same partials bit for bit; v recomputed inside the kernel that consumes it
    # (fd_pw_dw3x3_proj: LN -> W_v -> depthwise -> Weff[b] -> x + gate . ()) against the row-GEMM on the STORED v
    part3 = torch.empty_like(part1)
    L.call("fd_pw_dw3x3_gram", L.FD_BF16, xd.data_ptr(), Cin, 0, Cin, None, None, 1e-6, md.data_ptr(), md.data_ptr() + Cin * 4,
           6 * Cin, wpd.data_ptr(), wm.data_ptr(), None, 0, 0, part3.data_ptr(), B, H, W, s)
    torch.cuda.synchronize()
    assert torch.equal(part1, part3)
    assert L.lib().fd_pw_dw3x3_proj_ok(L.FD_BF16, Cin, H, W)
    e = eng_factory("bf16")
    weff = (torch.randn(B, 64, 64) / 8).to(HB.t).cuda()
    wm_v = DAEngine._dw_masked(wdw.reshape(192, 9)[128:].t().contiguous().cuda())
    vs = v[..., 8:].contiguous()
    ref = torch.empty(B, H, W, 64, device="cuda", dtype=HB.t)
    e.conv(None, vs, B, H, W, ref, c0=64, ld0=64, off0=0, weight=weff, w_batch_stride=64 * 64, bias=None, Cout=64, KH=1, KW=1,
           epi=L.EPI_GATE_RES, res=xd, gate=C.c_void_p(md.data_ptr() + 5 * Cin * 4), gate_ld=6 * Cin)
    got = torch.full((B, H, W, 64 + 8), 7.0, device="cuda", dtype=HB.t)
    L.call("fd_pw_dw3x3_proj", L.FD_BF16, xd.data_ptr(), Cin, 0, Cin, None, None, 1e-6, md.data_ptr(), md.data_ptr() + Cin * 4,
           6 * Cin, wpd.data_ptr() + 128 * Cin * 2, wm_v.data_ptr(), weff.data_ptr(), md.data_ptr() + 5 * Cin * 4, 6 * Cin,
           got.data_ptr(), 64 + 8, 8, B, H, W, s)
    torch.cuda.synchronize()
    assert float((got[..., :8].float() - 7.0).abs().max()) == 0.0
    assert torch.equal(got[..., 8:], ref)          # same operands, same rounding points, same MFMA order

@pytest.mark.parametrize("cfg", [dict(B=2, hw=(128, 256), cout=64), dict(B=12, hw=(144, 160), cout=64), dict(B=3, hw=(128, 256), cout=128)])
def test_gn_apply_down4x4(eng_factory, cfg):
    """fd_gn_apply_down4x4 (GroupNorm apply + SiLU + identity residual of a ResnetBlock and the 4x4 / stride-2
    convolution behind it in one pass; src/DADiff.py:128-131, 213-229, 418-430) against the two-pass HIP sequence
    fd_gn_silu_apply + fd_conv2d: the skip tensor bit for bit, the down-sampled tensor to fp32 summation order; and
    against torch.  The second case has a ragged last workgroup (45 tiles, two per workgroup)."""
    from founddiff_amd import _lib as L
    from founddiff_amd.engine import ConvW
    e = eng_factory("bf16")
    torch.manual_seed(51)
    B, (H, W), Co = cfg["B"], cfg["hw"], cfg["cout"]
    C_ = 64
    assert L.lib().fd_gn_apply_down4x4_ok(L.FD_BF16, C_, Co, H, W)
    bf = lambda t: t.to(HB.t).float()
    h = bf(torch.randn(B, H, W, C_) * 2 + 0.5)
    x = bf(torch.randn(B, H, W, C_))
    gam, bet = torch.randn(C_), torch.randn(C_)
    hv = h.reshape(B, H * W, 8, 8).permute(0, 2, 1, 3).reshape(B, 8, -1)
    mr = torch.stack([hv.mean(-1), torch.rsqrt(hv.var(-1, unbiased=False) + 1e-5)], -1).contiguous()
    wt, bias = bf(torch.randn(Co, C_, 4, 4) / 32), torch.randn(Co)
    cw = ConvW(wt, bias, e.dev, e.tdt)
    hd, xd, mrd, gd, bd = h.cuda().to(HB.t), x.cuda().to(HB.t), mr.cuda(), gam.cuda(), bet.cuda()
    s = torch.cuda.current_stream().cuda_stream
    # two passes
    sk0 = torch.empty(B, H, W, C_, device="cuda", dtype=HB.t)
    L.call("fd_gn_silu_apply", L.FD_BF16, hd.data_ptr(), mrd.data_ptr(), gd.data_ptr(), bd.data_ptr(), xd.data_ptr(),
           sk0.data_ptr(), B, H * W, C_, 8, s)
    o0 = torch.empty(B, H // 2, W // 2, Co, device="cuda", dtype=HB.t)
    e.conv(cw, sk0, B, H, W, o0, stride=2, pad=1)
    # one pass
    sk1 = torch.full((B, H, W, C_), 3.0, device="cuda", dtype=HB.t)
    o1 = torch.full((B, H // 2, W // 2, Co), 5.0, device="cuda", dtype=HB.t)
    L.call("fd_gn_apply_down4x4", L.FD_BF16, hd.data_ptr(), xd.data_ptr(), mrd.data_ptr(), gd.data_ptr(), bd.data_ptr(), 8,
           sk1.data_ptr(), cw.w.data_ptr(), cw.b.data_ptr(), o1.data_ptr(), B, H, W, C_, Co, s)
    torch.cuda.synchronize()
    assert torch.equal(sk0, sk1)
    assert rel_err(o1.float().cpu(), o0.float().cpu()) < 8e-3              # bf16 outputs of fp32 sums in two orders
    ref = F.conv2d(sk0.float().cpu().permute(0, 3, 1, 2), wt, bias, stride=2, padding=1).permute(0, 2, 3, 1)
    assert rel_err(o1.float().cpu(), ref) < 8e-3
    gn = F.group_norm(h.permute(0, 3, 1, 2), 8, gam, bet, 1e-5).permute(0, 2, 3, 1)
    assert rel_err(sk1.float().cpu(), x + F.silu(gn)) < 1.5e-2
    # deterministic
    o2 = torch.empty_like(o1)
    L.call("fd_gn_apply_down4x4", L.FD_BF16, hd.data_ptr(), xd.data_ptr(), mrd.data_ptr(), gd.data_ptr(), bd.data_ptr(), 8,
           sk1.data_ptr(), cw.w.data_ptr(), cw.b.data_ptr(), o2.data_ptr(), B, H, W, C_, Co, s)
    torch.cuda.synchronize()
    assert torch.equal(o1, o2)


@pytest.mark.parametrize("cfg", [(128, 64, 48), (256, 24, 32), (512, 8, 16)])
def test_dwconv_gram(eng_factory, cfg):
    """fd_dwconv_gram (qkv_dwconv of q, k -> L2 norms + q k^T, C >= 128; src/DADiff.py:267-276) against the unfused HIP pair
    fd_dwconv3x3 + fd_chan_attn_gram on the same qkv tensor, and the v slice through fd_dwconv3x3 with an offset."""
    from founddiff_amd import _lib as L
    from founddiff_amd.engine import DAEngine
    Cc, H, W = cfg
    torch.manual_seed(35)
    B = 2
    qkv = (torch.randn(B, H, W, 3 * Cc) * 0.7).to(HB.t).cuda()
    wdw = (torch.randn(9, 3 * Cc) / 3).cuda()
    wm = DAEngine._dw_masked(wdw)
    s = torch.cuda.current_stream().cuda_stream
    assert L.lib().fd_dwconv_gram_ok(L.FD_BF16, Cc, H, W)
    full = torch.empty(B, H, W, 3 * Cc, device="cuda", dtype=HB.t)
    L.call("fd_dwconv3x3", L.FD_BF16, qkv.data_ptr(), 3 * Cc, 0, wdw.data_ptr(), None, 0, full.data_ptr(), 3 * Cc, 0, B, H, W, 3 * Cc, s)
    nb0 = L.lib().fd_chan_attn_nblk(H * W)
    part0 = torch.empty(B, Cc // 32, nb0, 1088, device="cuda")
    L.call("fd_chan_attn_gram", L.FD_BF16, full.data_ptr(), B, H * W, Cc, part0.data_ptr(), s)
    nb1 = L.lib().fd_dwconv_gram_nblk(H, W)
    part1 = torch.full((B, Cc // 32, nb1, 1088), float("nan"), device="cuda")
    L.call("fd_dwconv_gram", L.FD_BF16, qkv.data_ptr(), 3 * Cc, Cc, wm.data_ptr(), part1.data_ptr(), B, H, W, s)
    v = torch.empty(B, H, W, Cc, device="cuda", dtype=HB.t)
    wv = wdw[:, 2 * Cc:].contiguous()
    L.call("fd_dwconv3x3", L.FD_BF16, qkv.data_ptr(), 3 * Cc, 2 * Cc, wv.data_ptr(), None, 0, v.data_ptr(), Cc, 0, B, H, W, Cc, s)
    torch.cuda.synchronize()
    assert torch.equal(v, full[..., 2 * Cc:])
    g0, g1 = part0.double().sum(2).cpu(), part1.double().sum(2).cpu()
    assert bool(torch.isfinite(g1).all())
    # the unfused pair rounds q, k to bf16 on their way through HBM (and its taps to bf16); fused, the depthwise runs on
    # packed fp16 and q, k stay fp16 on chip.  Both against the fp32 depthwise + Gram of the same qkv tensor: the fused
    # kernel is at least as close
    dwo = F.conv2d(qkv.float().cpu().permute(0, 3, 1, 2), wdw.cpu().t().reshape(3 * Cc, 1, 3, 3), None, padding=1, groups=3 * Cc)
    q = dwo[:, :Cc].reshape(B, Cc // 32, 32, H * W).double()
    k = dwo[:, Cc:2 * Cc].reshape(B, Cc // 32, 32, H * W).double()
    gram = (q @ k.transpose(-1, -2)).reshape(B, Cc // 32, 1024)
    e_f, e_u = rel_err(g1[..., :1024], gram), rel_err(g0[..., :1024], gram)
    # (on the binary16 build the unfused pair -- fp32-accumulating depthwise, q / k rounded to nearest -- is the closer one by a
    #  factor of two: the fused kernel's depthwise accumulates its nine taps in fp16; both far inside the gate)
    assert e_f < 4e-3 and (HB.fp16 or e_f < 1.5 * e_u + 1e-4), (e_f, e_u)
    assert rel_err(g1[..., 1024:1056], (q ** 2).sum(-1)) < 4e-3 and rel_err(g1[..., 1056:], (k ** 2).sum(-1)) < 4e-3
    assert rel_err(g1[..., :1024], g0[..., :1024]) < 8e-3
    part2 = torch.empty_like(part1)
    L.call("fd_dwconv_gram", L.FD_BF16, qkv.data_ptr(), 3 * Cc, Cc, wm.data_ptr(), part2.data_ptr(), B, H, W, s)
    torch.cuda.synchronize()
    assert torch.equal(part1, part2)


@pytest.mark.parametrize("cfg", [dict(cout=64, planes=2, hw=(48, 64)), dict(cout=32, planes=3, hw=(32, 32)),
                                 dict(cout=64, planes=1, hw=(16, 32))])
def test_init_conv7(eng_factory, cfg):
    """Dedicated init_conv kernel (7x7 from the fp32 planes, bf16) vs F.conv2d on bf16-rounded operands."""
    from founddiff_amd import _lib as L
    e = eng_factory("bf16")
    torch.manual_seed(41)
    B, (H, W), co, c = 2, cfg["hw"], cfg["cout"], cfg["planes"]
    x = torch.randn(B, c, H, W)
    w = torch.randn(co, c, 7, 7) / (7 * c ** 0.5)
    bias = torch.randn(co)
    # with <= 2 planes the kernel carries the planes as bf16 hi + lo pairs: the image is NOT rounded to bf16
    ref = F.conv2d(x if c <= 2 else rq(x, "bf16"), rq(w, "bf16"), bias, padding=3)
    assert L.lib().fd_init_conv7_ok(L.FD_BF16, co, H, W)
    wp = e._pack_init7(w)
    planes = [x[:, i].contiguous().cuda() for i in range(c)] + [None] * (3 - c)
    out = torch.empty(B, H, W, co, device="cuda", dtype=HB.t)
    bd = bias.cuda()
    L.call("fd_init_conv7", L.FD_BF16, *[None if p is None else p.data_ptr() for p in planes], wp.data_ptr(),
           bd.data_ptr(), out.data_ptr(), B, H, W, co, None)
    torch.cuda.synchronize()
    assert rel_err(nchw(out), ref) < 4e-3          # output rounding to bf16 only
    assert rel_err(nchw(out)[:, :, :3], ref[:, :, :3]) < 6e-3 and rel_err(nchw(out)[..., -3:], ref[..., -3:]) < 6e-3


@pytest.mark.parametrize("cfg", [
    dict(c0=128, c1=0, cout=128, hw=(64, 64)),                 # <128,8>: 2 x 2 waves
    dict(c0=256, c1=0, cout=64, hw=(64, 64)),                  # <64,16>
    dict(c0=64, c1=64, cout=64, hw=(72, 64)),                  # <64,8>, two sources inside one 128-channel slab
    dict(c0=256, c1=128, cout=200, hw=(64, 64)),               # three slabs, second source, ragged Cout
    dict(c0=128, c1=0, cout=64, hw=(32, 32), up=True),         # nearest x2 up-sampling in the halo index map
])
def test_conv3x3_fp8_weights(eng_factory, cfg):
    """BASELINE configs[4]: e4m3 weights (one scale per output channel) on v_mfma_scale_f32_16x16x128_f8f6f4 in the
    3x3 halo kernel.  Checked EXACTLY against the same arithmetic on the CPU: activations x act_scale -> e4m3,
    weights / scale -> e4m3, fp32 products and sums -- what remains is the accumulation order and the bf16 rounding
    of the output.  Also against the unquantised conv within the e4m3 rounding noise."""
    from founddiff_amd import engine as E
    e = eng_factory("fp8")
    e.fp8 = True
    torch.manual_seed(3)
    B = 2
    H, W = cfg["hw"]
    c0, c1, co = cfg["c0"], cfg["c1"], cfg["cout"]
    cin = c0 + c1
    up = cfg.get("up", False)
    x = (torch.randn(B, cin, H, W) * 1.5).to(HB.t).float()
    w = torch.randn(co, cin, 3, 3) / (3 * cin ** 0.5)
    bias = torch.randn(co) * 0.1
    cw = E.ConvW(w, bias, "cuda", HB.t, fp8=True)
    assert cw.w8 is not None and cw.w8.dtype == torch.float8_e4m3fn
    a_s = E.FP8_ACT_SCALE
    xq = (x * a_s).clamp(-448, 448).to(torch.float8_e4m3fn).float() / a_s
    wq = (cw.w8.float().cpu() * cw.ws.cpu()[:, None]).reshape(co, 3, 3, cin).permute(0, 3, 1, 2)
    xin = F.interpolate(xq, scale_factor=2, mode="nearest") if up else xq
    ref = F.conv2d(xin, wq, bias, padding=1)
    full = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest") if up else x, w, bias, padding=1)
    xd = nhwc(x, HB.t)
    a, b = (xd[..., :c0].contiguous(), xd[..., c0:].contiguous()) if c1 else (xd, None)
    OH, OW = (2 * H, 2 * W) if up else (H, W)
    out = torch.empty(B, OH, OW, co, device="cuda", dtype=HB.t)
    kw = dict(c0=c0, in1=b, c1=c1, upsample=up)
    assert e.conv(cw, a, B, H, W, out, probe="kid", **kw) == 12
    e.conv(cw, a, B, H, W, out, **kw)
    torch.cuda.synchronize()
    assert rel_err(nchw(out), ref) < 6e-3                     # bf16 output rounding only
    assert float((nchw(out) - full).norm() / full.norm()) < 6e-2      # e4m3 rounding of both operands
    # same conv with GroupNorm partial sums: the fp8 form feeds the same statistics workspace
    mt = L_mtiles(OH, OW)
    part = torch.zeros(B, mt, co, 2, device="cuda")
    e.conv(cw, a, B, H, W, out, stats=part, **kw)
    torch.cuda.synchronize()
    s = part.sum(1).cpu()
    got = nchw(out)
    assert torch.allclose(s[..., 0], got.sum((2, 3)), rtol=2e-2, atol=2.0)


def L_mtiles(OH, OW):
    from founddiff_amd import _lib as L
    return L.lib().fd_conv_mtiles(OH, OW)


@pytest.mark.parametrize("cfg", [(128, 4, 4, 32, 48), (128, 8, 4, 16, 16), (256, 16, 8, 16, 32), (256, 8, 8, 32, 16), (128, 4, 4, 15, 21),
                                 (64, 4, 4, 8, 8)])
def test_selective_scan_fused_xproj(cfg):
    """fd_selective_scan_xproj: the x_proj einsum (src/emamba2.py:332) inside the scan's first phase (bf16, one
    workgroup per chunk) -- x_dbl rows and y against the CPU einsum + sequential oracle, incl. an odd image."""
    from founddiff_amd import _lib as L
    from oracle import nets
    D, N, R, H, W = cfg
    assert L.lib().fd_selective_scan_fuses_xproj(L.FD_BF16, D, N, R) == 1
    assert L.lib().fd_selective_scan_fuses_xproj(L.FD_BF16, 512, 32, 16) == 0 and L.lib().fd_selective_scan_fuses_xproj(L.FD_F32, D, N, R) == 0
    torch.manual_seed(8)
    B, CD = 2, R + 2 * N
    H2, W2 = (H + 1) // 2, (W + 1) // 2
    Lq = H2 * W2
    xc = (torch.randn(B, D, H, W) * 0.5).to(HB.t).float()
    xw = (torch.randn(4, CD, D) / D ** 0.5).to(HB.t).float()
    dtw = (torch.rand(4, D, R) * 2 - 1) * R ** -0.5
    dtb = torch.randn(4, D) * 0.5 - 3
    A = -torch.exp(torch.log(torch.arange(1, N + 1).float())[None].repeat(4 * D, 1) + 0.1 * torch.randn(4 * D, N))
    Ds = 1 + 0.1 * torch.randn(4 * D)
    # the CPU einsum + sequential oracle; x_dbl rows at row index h2 * W2 + w2 whatever the direction's scan order
    ref, xd_rows = scan_reference(xc, dtw, dtb, A, Ds, N, R, xw=xw, scan_fn=nets.selective_scan)
    ws = torch.empty(L.lib().fd_scan_ws_floats(B, H, W, D, N), device="cuda")
    y = torch.empty(B, H, W, D, device="cuda", dtype=HB.t)
    xdbl = torch.full((4, B, Lq, CD), float("nan"), device="cuda")
    t = [v.contiguous().cuda() for v in (dtw, dtb, A, Ds)]
    xcd, xwd = nhwc(xc, HB.t), xw.to("cuda", HB.t).contiguous()
    L.call("fd_selective_scan_xproj", L.FD_BF16, xcd.data_ptr(), xwd.data_ptr(), xdbl.data_ptr(), t[0].data_ptr(), t[1].data_ptr(),
           t[2].data_ptr(), t[3].data_ptr(), y.data_ptr(), ws.data_ptr(), B, H, W, D, N, R, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rel_err(xdbl.cpu(), xd_rows) < 1e-5
    assert rel_err(nchw(y), ref) < 1e-2


def test_integration_recipe_for_the_reference_extension():
    """the reference imports its native op as
    `from selective_scan_vmamba_pt202 import selective_scan_cuda_core` (src/emamba2.py:27) and calls
    `selective_scan_cuda_core.fwd(u, delta, A, B, C, D, delta_bias, delta_softplus, nrows)` (154).  With the two
    sys.modules entries of the recipe that import resolves to this library and the reference's own call pattern
    (SelectiveScan.forward, 124-157: contiguity fix-ups, 3-D B/C un-squeezed, `out, x, *rest = ...`) runs unchanged."""
    import importlib
    import sys
    import types
    from oracle import nets
    import founddiff_amd.selective_scan_cuda_core as ssc
    saved = {k: sys.modules.get(k) for k in ("selective_scan_cuda_core", "selective_scan_vmamba_pt202")}
    try:
        sys.modules["selective_scan_cuda_core"] = ssc
        pkg = types.ModuleType("selective_scan_vmamba_pt202")
        pkg.selective_scan_cuda_core = ssc
        sys.modules["selective_scan_vmamba_pt202"] = pkg
        core = importlib.import_module("selective_scan_vmamba_pt202").selective_scan_cuda_core     # what line 27 binds
        u, delta, A, Bm, Cm, D, bias = _scan_inputs(2, 64, 1, 8, 300, seed=21)
        ud, dd = u.cuda().transpose(1, 2).contiguous().transpose(1, 2), delta.cuda()      # a non-contiguous u, as 134-135 guards
        if ud.stride(-1) != 1:
            ud = ud.contiguous()
        B3, C3 = Bm[:, 0].cuda(), Cm[:, 0].cuda()                                          # 3-D B / C: 144-149
        out, x, *rest = core.fwd(ud, dd, A.cuda(), B3.unsqueeze(1), C3.unsqueeze(1), D.cuda(), bias.cuda(), True, 1)
        assert rest == [] and x.shape == (2, 64, 8)
        ref = nets.selective_scan(u, delta, A, Bm[:, :1], Cm[:, :1], D, bias, softplus=True)
        assert rel_err(out.cpu(), ref) < 1e-5
        with pytest.raises(NotImplementedError):
            core.bwd()
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
