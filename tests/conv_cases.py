"""The shapes of tests/test_gpu_conv_forms.py, and the fp64 restatement of fd_conv2d they are compared with.

fd_conv2d sends a dense contraction to one of eighteen kernels (fd_conv_kernel_id).  Ids 0 .. 6 are the seven tile shapes of the generic
implicit-GEMM kernel (conv_igemm_kernel, csrc/fd_conv.hip), each compiled in four forms: bf16 with the pointwise loader (PW), bf16 with
the general gather, fp32, and fp32 with the split-bf16 contraction.  CONV_CASES is chosen to reach every one of the 28, every edge of
the M / N / K tiling, every operand and output layout and every epilogue in both of its code paths; tests/test_conv_forms_cpu.py
asserts that from fd_conv_form's answers (no GPU), so a case cannot be dropped, or a threshold of the dispatcher moved, without the
coverage test naming what lost its test."""
import ctypes as C
from collections import namedtuple

import torch
import torch.nn.functional as F

FD_F32, FD_BF16 = 0, 1
EPIS = ("NONE", "SILU_SPLIT", "RELU", "GATE_RES", "RES_RELU", "GNSILU_ADD")          # value = index (include/founddiff_hip.h)
ALL = ("bf16", "fp32", "fp32s")       # 'bf16': the build's 16-bit type; 'fp32': exact-f32 MFMA; 'fp32s': fp32 storage, split-bf16
# (BM, BN, WM, WN) of the tile ids 0 .. 6 (csrc/fd_conv.hip: FD_CONV_DISPATCH)
TILES = {0: (128, 128, 2, 2), 1: (128, 64, 2, 2), 2: (64, 128, 2, 2), 3: (64, 64, 2, 2), 4: (128, 256, 2, 4), 5: (256, 256, 4, 2),
         6: (128, 32, 2, 2)}

# geometry: B, source H x W, kernel k (square), stride, pad, nearest x2 up-sampling, ndir (4: the SS2D sub-grids; OH / OW given)
# sources:  cin = c0 + c1 channels, the first c0 from source 0 (pixel stride ld0, channel offset off0), the rest from source 1
# slices:   output pixel stride ldo / offset offo, out_f32, residual ld_res / off_res, gate_ld; wb: per-image weights
# epilogue: epi (a name of EPIS), split, groups (GNSILU_ADD); stats: GroupNorm partial sums wanted
# expect:   kid, and pw = the 16-bit mode runs the pointwise loader (fd_conv_form; the fp32 modes have no such loader)
Case = namedtuple("Case", "name B H W k stride pad up ndir OH OW cin c1 ld0 off0 ld1 off1 cout ldo offo out_f32 bias wb epi split "
                          "groups gate_ld ld_res off_res stats modes expect")


def _c(name, B, hw, cin, cout, k=1, stride=1, pad=None, up=False, ndir=1, c1=0, ld0=None, off0=0, ld1=None, off1=0, ldo=None, offo=0,
       out_f32=False, bias=True, wb=False, epi="NONE", split=0, groups=0, gate_ld=None, ld_res=None, off_res=0, stats=False, modes=ALL,
       **expect):
    H, W = hw
    pad = (k - 1) // 2 if pad is None else pad
    if ndir == 4:          # the engine's x_proj: sub-grids of the image zero-padded to even sizes
        OH, OW = (H + 1) // 2, (W + 1) // 2
    else:
        Hs, Ws = (2 * H, 2 * W) if up else (H, W)
        OH, OW = (Hs + 2 * pad - k) // stride + 1, (Ws + 2 * pad - k) // stride + 1
    c0 = cin - c1
    assert epi in EPIS and set(expect) == {"kid", "pw"}
    return Case(name, B, H, W, k, stride, pad, up, ndir, OH, OW, cin, c1, ld0 or c0, off0, ld1 or c1, off1, cout, ldo or cout, offo,
                out_f32, bias, wb, epi, split, groups, gate_ld or cout, ld_res or cout, off_res, stats, tuple(modes), expect)


TALL = (130, 127)        # 16510 output pixels = 128 * 128 + 126: 128-row tiles, the last one partly full, its second band 62 rows
TALL_E = (139, 118)      # 16402 = 128 * 128 + 18: the last tile's second 64-row band is empty (257 bands)

CONV_CASES = [
    # ---- 128-row tiles (more than 16384 output pixels): ids 0, 1, 6
    # id 0 through the pointwise loader: two sources joined on a K-tile boundary, both slices of wider tensors; K = 320 (the streaming
    # row-GEMM stops at 256); Cout 96 of a 128-column tile
    _c("tall-pw-96", 1, TALL, 320, 96, c1=128, ld0=200, off0=8, ld1=136, off1=8, kid=0, pw=1),
    # id 0 through the general gather: Cin 96 at 3x3 -- K tiles that straddle a tap beside tiles on the counter path; GroupNorm sums
    # of a 128-row tile with a ragged last band, over ReLU's output
    _c("tall-3x3-96-relu-stats", 1, TALL, 96, 96, k=3, epi="RELU", stats=True, kid=0, pw=0),
    _c("tall-e-3x3-72-stats", 1, TALL_E, 16, 72, k=3, stats=True, kid=0, pw=0),
    # id 1, pointwise loader + direct epilogue: gated residual, fp32 output from 16-bit operands, residual and gate in wider rows
    _c("tall-pw-64-gate-f32", 1, TALL, 64, 64, out_f32=True, epi="GATE_RES", gate_ld=80, ld_res=72, off_res=8, kid=1, pw=1),
    # id 1, general: Cin 32 (half a K tile in 16 bits); sums with an empty last band, over a SiLU that starts inside an 8-channel vector
    _c("tall-e-40-silu20-stats", 1, TALL_E, 32, 40, epi="SILU_SPLIT", split=20, stats=True, kid=1, pw=0),
    # id 6 through the pointwise loader: one 16-channel MFMA tile per wave, so the accumulators go through the LDS-staged epilogue
    _c("tall-pw-24-gnsilu", 1, TALL, 64, 24, epi="GNSILU_ADD", groups=3, kid=6, pw=1),
    _c("tall-pw-32-resrelu-slices", 1, TALL, 128, 32, ldo=48, offo=8, out_f32=True, epi="RES_RELU", ld_res=40, off_res=8, kid=6, pw=1),
    # the production x_proj: four stride-2 sub-grids of an image with an odd number of rows, Cout 12 in fp32 through the scalar epilogue
    _c("tall-xproj-12", 1, (259, 254), 64, 12, stride=2, pad=0, ndir=4, out_f32=True, bias=False, kid=6, pw=0),
    # id 6 with sums: 4x4 stride 2 pad 1, Cin 8 (a K tile spans eight taps)
    _c("tall-4x4s2-16-stats", 1, (260, 254), 8, 16, k=4, stride=2, pad=1, stats=True, kid=6, pw=0),
    # ---- the 8-wave tiles of images up to 16384 pixels: ids 4 and 5 (workgroup-count thresholds of 192)
    _c("id4-pw-512-silu", 2, (78, 79), 256, 512, epi="SILU_SPLIT", split=256, kid=4, pw=1),
    _c("id5-pw-512-resrelu", 2, (110, 110), 256, 512, epi="RES_RELU", kid=5, pw=1),
    _c("id4-3x3-264", 2, (78, 79), 32, 264, k=3, kid=4, pw=0),
    _c("id5-3x3-264-gate", 2, (110, 110), 32, 264, k=3, epi="GATE_RES", kid=5, pw=0),
    # ---- 64-row tiles: ids 2 and 3
    _c("pw-136-silu64", 2, (9, 13), 128, 136, c1=64, epi="SILU_SPLIT", split=64, kid=2, pw=1),
    _c("pw-128-gnsilu", 2, (10, 10), 64, 128, epi="GNSILU_ADD", groups=8, kid=2, pw=1),
    _c("up-3x3-72-resrelu", 2, (6, 10), 32, 72, k=3, up=True, epi="RES_RELU", ld_res=80, off_res=8, kid=2, pw=0),
    _c("3x3-200-stats", 2, (8, 8), 128, 200, k=3, stats=True, kid=2, pw=0),
    _c("pw-40-relu", 2, (5, 7), 64, 40, epi="RELU", kid=3, pw=1),
    _c("pw-64-f32-slices", 2, (9, 13), 64, 64, ld0=96, off0=32, ldo=96, offo=16, out_f32=True, kid=3, pw=1),
    _c("pw-64-gate", 2, (12, 10), 128, 64, c1=64, ld1=72, off1=8, epi="GATE_RES", gate_ld=72, ld_res=72, off_res=8, kid=3, pw=1),
    _c("pw-64-resrelu", 2, (7, 9), 64, 64, epi="RES_RELU", kid=3, pw=1),
    # 7x7 pad 3, Cin 8, Cout 4: the scalar epilogue below one vector; sums at BM 64 (two passes per band)
    _c("7x7-4-stats", 2, (11, 9), 8, 4, k=7, stats=True, kid=3, pw=0),
    # the c0 boundary inside a K tile of either width (Cin 48 = 40 + 8), sums over a gated residual's output, output slice of a wider fp32 tensor
    _c("cat-3x3-64-gate-stats", 2, (12, 10), 48, 64, k=3, c1=8, ld0=56, off0=8, ld1=24, off1=8, ldo=96, offo=16, out_f32=True,
       epi="GATE_RES", gate_ld=72, ld_res=72, off_res=8, stats=True, kid=3, pw=0),
    _c("4x4s2-128", 2, (16, 24), 64, 128, k=4, stride=2, pad=1, kid=2, pw=0),
    _c("wbatch-32-gate", 2, (12, 10), 32, 32, ld0=96, off0=64, bias=False, wb=True, epi="GATE_RES", gate_ld=50, kid=3, pw=0),
    _c("xproj-tiny-12", 2, (7, 10), 64, 12, stride=2, pad=0, ndir=4, out_f32=True, bias=False, kid=3, pw=0),
] + [
    # ---- every epilogue through the LDS-staged path, on 8-channel vectors (Cout 24) and element by element (Cout 20)
    _c(f"3x3-{co}-{e.lower()}", 2, (6, 7), 16, co, k=3, epi=e, split=12, groups=4, ld_res=co + (8 if co % 8 == 0 else 3),
       off_res=(8 if co % 8 == 0 else 3), kid=3, pw=0) for co in (24, 20) for e in EPIS
]

# batch invariance across tiles: (case at B = 2, the id its B = 1 twin runs on)
BATCH_CASES = [
    (_c("inv-4-none", 2, (78, 79), 256, 512, bias=False, kid=4, pw=1), 2),
    (_c("inv-4-gate", 2, (78, 79), 256, 512, epi="GATE_RES", kid=4, pw=1), 2),
    (_c("inv-5-none", 2, (110, 110), 256, 512, bias=False, kid=5, pw=1), 2),
    (_c("inv-5-silu", 2, (110, 110), 256, 512, epi="SILU_SPLIT", split=256, kid=5, pw=1), 2),
]
BATCH_MODES = ("bf16", "fp32")

# the pointwise loader against the general gather: the same 1x1 problem with its K axis over one source (PW) or split at channel 72
# (c0 not a multiple of 64: general, same K order)
PW_GENERAL_CASES = [_c(f"pwgen-{kid}-{e.lower()}", B, hw, 128, co, epi=e, groups=gr, kid=kid, pw=1)
                    for B, hw, co, gr, kid in ((2, (9, 13), 64, 4, 3), (2, (9, 13), 160, 4, 2), (1, TALL, 72, 3, 0), (1, TALL, 24, 3, 6))
                    for e in ("NONE", "GATE_RES", "GNSILU_ADD")]


def split_sources(c, t, c0=72):
    """the same problem with its K axis over two sources: both are the one source tensor, read from channel 0 and from channel c0"""
    assert c.c1 == 0 and c.off0 == 0 and c.ld0 == c.cin
    c2 = c._replace(c1=c.cin - c0, ld1=c.cin, off1=c0, expect=dict(c.expect, pw=0))
    return c2, dict(t, in1=t["in0"])


def case_id(c):
    return c.name


def ohw(c):
    return c.OH * c.OW


def bands(c):
    return -(-ohw(c) // 64)


def expected_form(c, mode):
    return c.expect["kid"] | ((c.expect["pw"] if mode == "bf16" else 0) << 8)


def tile_geom(c, mode, form):
    """what the kernel's template parameters make of (case, mode) on the tile fd_conv_form named"""
    kid, pw = form & 0xFF, form >> 8
    BM, BN, WM, WN = TILES[kid]
    NT = BN // WN // 16
    return dict(kid=kid, pw=pw, BM=BM, BN=BN, TMW=BM // WM, BK=64 if mode == "bf16" else 32, pwe=bool(pw) and NT % 2 == 0,
                K=c.k * c.k * c.cin)


def vec_ok(c):
    """the staged epilogue's 8-channel vector form (csrc/fd_conv.hip: vec_ok)"""
    has_res = c.epi in ("GATE_RES", "RES_RELU")
    return c.cout % 8 == 0 and c.ldo % 8 == 0 and c.offo % 8 == 0 and (not has_res or (c.ld_res % 8 == 0 and c.off_res % 8 == 0))


def k_paths(c, BK):
    """the general loader's K-tile walk (gload): which of its two address paths the tiles of one launch take -- 'counter' (the tile
    lies inside one filter tap: no division) or 'decode' (it straddles taps or runs past K)"""
    K, cin = c.k * c.k * c.cin, c.cin
    paths, t_cb = set(), 0
    for _ in range(-(-K // BK)):
        paths.add("counter" if t_cb + BK <= cin else "decode")
        t_cb += BK
        while t_cb >= cin:
            t_cb -= cin
    return paths


def params_for(c, mode, ptrs):
    """fd_conv_params of (case, mode).  ptrs: name -> address for in0, in1, weight, bias, out, res, gate, h, gn, gamma, beta, stats
    (what the case does not use is ignored)"""
    from founddiff_amd import _lib as L
    p = L.ConvParams()
    K = c.k * c.k * c.cin
    p.dtype, p.out_f32 = (FD_BF16 if mode == "bf16" else FD_F32), int(c.out_f32)
    p.f32_split = int(mode == "fp32s")
    p.in0, p.c0, p.ld0, p.off0 = ptrs["in0"], c.cin - c.c1, c.ld0, c.off0
    if c.c1:
        p.in1, p.c1, p.ld1, p.off1 = ptrs["in1"], c.c1, c.ld1, c.off1
    p.B, p.H, p.W, p.upsample = c.B, c.H, c.W, int(c.up)
    p.KH, p.KW, p.stride, p.pad_h, p.pad_w = c.k, c.k, c.stride, c.pad, c.pad
    p.OH, p.OW, p.ndir = c.OH, c.OW, c.ndir
    p.weight = ptrs["weight"]
    p.w_batch_stride = c.ndir * c.cout * K if c.wb else 0
    p.w_dir_stride = c.cout * K if c.ndir > 1 else 0
    p.bias = ptrs["bias"] if c.bias else None
    p.Cout, p.out, p.ldo, p.offo = c.cout, ptrs["out"], c.ldo, c.offo
    p.out_dir_stride = c.B * ohw(c) * c.ldo if c.ndir > 1 else 0
    p.epilogue, p.epi_split = EPIS.index(c.epi), c.split
    p.ld_res, p.off_res, p.gate_ld, p.gn_groups = c.ld_res, c.off_res, c.gate_ld, max(c.groups, 1)
    if c.epi in ("GATE_RES", "RES_RELU"):
        p.res = ptrs["res"]
    if c.epi == "GATE_RES":
        p.gate = ptrs["gate"]
    if c.epi == "GNSILU_ADD":
        p.h, p.gn_mean_rstd, p.gn_gamma, p.gn_beta = ptrs["h"], ptrs["gn"], ptrs["gamma"], ptrs["beta"]
    if c.stats:
        p.stats_partial = ptrs["stats"]
    return p


DUMMY_PTRS = {n: 0x10000 * (i + 1) for i, n in enumerate("in0 in1 weight bias out res gate h gn gamma beta stats".split())}


def form(lib, c, mode, ptrs=None):
    return int(lib.fd_conv_form(C.byref(params_for(c, mode, ptrs or DUMMY_PTRS))))


def make_inputs(c, rq, seed=11):
    """the operands of one call on the CPU in fp32, in the layouts fd_conv_params describes.  rq rounds what the library stores in
    its element type (sources, weights, residual, h) to that type; bias, gate and the GroupNorm operands are fp32 in every mode."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    K, P = c.k * c.k * c.cin, ohw(c)
    t = dict(in0=rq(rn(c.B, c.H, c.W, c.ld0)))
    if c.c1:
        t["in1"] = rq(rn(c.B, c.H, c.W, c.ld1))
    t["weight"] = rq(rn(c.B if c.wb else 1, c.ndir, c.cout, K) / K ** 0.5)       # [image][direction][Cout][K], K order (kh, kw, c)
    if c.bias:
        t["bias"] = rn(c.cout)
    if c.epi in ("GATE_RES", "RES_RELU"):
        t["res"] = rq(rn(c.ndir, c.B, P, c.ld_res))
    if c.epi == "GATE_RES":
        t["gate"] = rn(c.B, c.gate_ld)
    if c.epi == "GNSILU_ADD":
        h = rq(rn(c.B, P, c.cout) * 1.5 + 0.5)
        hv = h.view(c.B, P, c.groups, c.cout // c.groups).permute(0, 2, 1, 3).reshape(c.B, c.groups, -1)
        t["h"] = h
        t["gn"] = torch.stack([hv.mean(-1), torch.rsqrt(hv.var(-1, unbiased=False) + 1e-5)], -1).contiguous()
        t["gamma"], t["beta"] = 1 + 0.2 * rn(c.cout), 0.3 * rn(c.cout)
    return t


def batch_slice(c, t, i):
    """(case, operands) of image i alone"""
    keep = {"bias", "gamma", "beta"}
    sl = {k: (v if k in keep else (v[:, i:i + 1] if k == "res" else (v[i:i + 1] if k != "weight" or c.wb else v))) for k, v in t.items()}
    return c._replace(B=1), sl


def gather_operand(c, t):
    """step 1: the A operand of every direction, explicitly: channel slices of the two sources concatenated, nearest x2 up-sampling,
    and for ndir = 4 the sub-grid with origin (k & 1, k >> 1) of the image zero-filled outside (what the loader's bounds check does).
    -> list over directions of (x [B, Cin, h, w] fp64, stride, pad)"""
    c0 = c.cin - c.c1
    x = t["in0"][..., c.off0:c.off0 + c0]
    if c.c1:
        x = torch.cat((x, t["in1"][..., c.off1:c.off1 + c.c1]), -1)
    x = x.permute(0, 3, 1, 2).double()
    if c.up:
        x = x.repeat_interleave(2, 2).repeat_interleave(2, 3)
    if c.ndir == 1:
        return [(x, c.stride, c.pad)]
    assert c.k == 1
    xp = F.pad(x, (0, c.stride * c.OW + 1 - x.shape[3], 0, c.stride * c.OH + 1 - x.shape[2]))
    return [(xp[:, :, (d & 1):(d & 1) + c.stride * c.OH:c.stride, (d >> 1):(d >> 1) + c.stride * c.OW:c.stride], 1, 0) for d in range(4)]


def conv_reference(c, t):
    """fd_conv2d restated in fp64 on the CPU: gather, F.conv2d, epilogue, band sums.  Returns a dict of fp64 tensors shaped
    [ndir, B, OH*OW, Cout] (gate / L broadcast): out; S = the same convolution of |x| with |w|, + |bias|; L = the epilogue's Lipschitz
    factor with respect to the contraction; addend = what the epilogue adds (residual or GroupNorm-SiLU term); and for the stats
    sum / sq [B, bands, Cout] with abs = the band sums of |out|."""
    P = ohw(c)
    outs, Ss = [], []
    for d, (x, stride, pad) in enumerate(gather_operand(c, t)):
        od, sd = [], []
        for b in range(c.B):
            w = t["weight"][b if c.wb else 0, d].double().view(c.cout, c.k, c.k, c.cin).permute(0, 3, 1, 2)
            od.append(F.conv2d(x[b:b + 1], w, None, stride=stride, padding=pad))
            sd.append(F.conv2d(x[b:b + 1].abs(), w.abs(), None, stride=stride, padding=pad))
        o, s = torch.cat(od), torch.cat(sd)
        assert o.shape[2:] == (c.OH, c.OW), (c.name, o.shape)
        outs.append(o.permute(0, 2, 3, 1).reshape(c.B, P, c.cout))
        Ss.append(s.permute(0, 2, 3, 1).reshape(c.B, P, c.cout))
    v, S = torch.stack(outs), torch.stack(Ss)
    if c.bias:
        v, S = v + t["bias"].double(), S + t["bias"].double().abs()
    L, addend = torch.ones(1, 1, 1, c.cout, dtype=torch.float64), torch.zeros_like(v)
    silu = lambda z: z * torch.sigmoid(z)
    if c.epi == "RELU":
        out = v.clamp(min=0)
    elif c.epi == "SILU_SPLIT":
        out = torch.cat((v[..., :c.split], silu(v[..., c.split:])), -1)
        L = torch.where(torch.arange(c.cout) >= c.split, 1.1, 1.0).double().view(1, 1, 1, -1)
    elif c.epi in ("GATE_RES", "RES_RELU"):
        addend = t["res"][..., c.off_res:c.off_res + c.cout].double()
        if c.epi == "GATE_RES":
            gate = t["gate"][:, :c.cout].double().view(1, c.B, 1, c.cout)
            out, L = addend + gate * v, gate.abs()
        else:
            out = (v + addend).clamp(min=0)
    elif c.epi == "GNSILU_ADD":
        mr = t["gn"].double().repeat_interleave(c.cout // c.groups, 1)                 # [B, Cout, 2]
        addend = silu((t["h"].double() - mr[:, None, :, 0]) * mr[:, None, :, 1] * t["gamma"].double() + t["beta"].double())[None]
        out = v + addend
    else:
        out = v
    r = dict(out=out, S=S, L=L, addend=addend.abs())
    if c.stats:
        r.update(sum=band_sum(c, out), sq=band_sum(c, out * out), abs=band_sum(c, out.abs()))
    return r


def band_sum(c, z):
    """[1, B, OH*OW, Cout] -> per-channel sums over the 64-pixel bands of each image, [B, bands, Cout]"""
    nb = bands(c)
    return F.pad(z[0], (0, 0, 0, nb * 64 - ohw(c))).view(c.B, nb, 64, c.cout).sum(2)


U_OUT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -24}


def c_mode(c, mode):
    """relative error of the contraction per unit of S.  fp32 and the 16-bit modes: (K + 8) 2^-24 -- products of pre-rounded 16-bit
    operands are exact in fp32 (8 + 8 and 11 + 11 significand bits), so only the accumulation rounds.  fp32s: + 2^-14 for the dropped
    lo.lo term and the two roundings of lo."""
    K = c.k * c.k * c.cin
    return (K + 8) * 2.0 ** -24 + (2.0 ** -14 if mode == "fp32s" else 0.0)


def error_bounds(c, mode, ref, out_dtype):
    """(bound of a stored element, bound of the fp32 value before the store rounding), from the inputs alone:
    u_out |ref| + L c_mode S + 2^-20 (|ref| + |addend|); the last term is the fp32 epilogue arithmetic and the fast exponential."""
    pre = ref["L"] * c_mode(c, mode) * ref["S"] + 2.0 ** -20 * (ref["out"].abs() + ref["addend"])
    return U_OUT[out_dtype] * ref["out"].abs() + pre, pre
