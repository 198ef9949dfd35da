"""The shapes of tests/test_gpu_pwdw_forms.py, and the fp64 restatement of the fused LayerNorm + modulate -> 1x1 -> depthwise 3x3 family
they are compared with (csrc/fd_pwdw.hip: pwdw_kernel<64>, <128>, <64, PROJ>, pwdw_gram_kernel, dwconv_gram_kernel; csrc/fd_pwdw32.hip:
pwdw32_kernel<DW, 16>, <GRAM, 8>, <PROJ, 8>).  Which kernel a launch runs, how many consecutive tiles a workgroup walks and on which grid
is fd_pw_dw3x3_plan's answer (host only); tests/test_pwdw_forms_cpu.py asserts from it what CASES reach.

Shapes are the smallest the kernels accept (32768 px for the 16-bit kernels, 16384 px for the fp32-storage ones, no floor for
fd_dwconv_gram), chosen by their tile counts: one tile row, one tile column, counts that leave 3 and 1 tiles to the last workgroup, and
an exact one.  The development switches are compiled away in the tested build: the tiles per workgroup they override are unreachable.

Reference (pwdw_reference): fp64 on the device, from the operands' STORED values -- x in the build's 16-bit type (fp32 for the
fp32-storage kernels), the 1x1 weights as stored (hi + lo), the taps as the fp16 pairs handed over (fp32):
    xn = LN(x) G + Bc (biased variance; rows_cases.prologue)        t = W xn        t = 0 outside the image (the conv pads ITS input)
    y = sum_tap w_tap t_tap + b      out_dw = y or SiLU(y)      z = SiLU(W_z xn)      PROJ: out = x + gate (Weff[b] y)
    Gram: per head q k^T, sum q^2, sum k^2 over the pixels of each WORKGROUP's own tiles (the plan says which), not over the image:
    a skipped or doubled tile shows.

The bound (error_bounds), derived from the formats and the kernels' rounding points, never fitted to a kernel's output:
  1x1 tile, per halo pixel   dt = u_t |t| + eta + (K + 8) 2^-24 S_t + S_pro   (+ 2^-14 S_t in fp32s: rows_cases.c_mode's split term)
      S_t = sum |w| |xn|;  S_pro = sum |w| (u_h |xn| + C_LN abar), rows_cases' prologue term (u_h: xn packed to 16 bits; 0 in fp32s)
      u_t: unit roundoff of the on-chip fp16 tile -- 2^-10 on the default build (v_cvt_pkrtz_f16_f32 rounds toward zero: pk_h2),
      2^-11 on the binary16 build (round to nearest), 0 in fp32s (the tile is fp32)
      eta = 2^-24: fp16's subnormal spacing, 16-bit kernels only.  It assumes the conversion KEEPS fp16 subnormals; the range-lo cases
      (1x1 output ~1e-5, inside the subnormal range) decide it: a flushing conversion would miss this bound by orders of magnitude
      (the term would have to be 2^-14).  On an MI355X they pass on both builds: subnormals are kept, as the comment in
      dwconv_gram_kernel's halo_store ("below 6.1e-5 become fp16 subnormals, below ~3e-8 zero") and the header's note on q / k say.
      fd_dwconv_gram reads stored q / k: dt = eta alone (bf16 -> fp16 is exact inside fp16's range: h16_to_h2).
  LayerNorm: C_LN = 4 x C_LN_MEASURED x (1 + RATIO_MAX^2).  C_LN_MEASURED is fp32 torch against fp64 on this table's own inputs
      (measure_c_ln, on the CPU, never the kernel); the 16-bit kernels take the variance in ONE pass (fd_ln_mod_chunk), whose relative
      error carries the factor 1 + (mean / std)^2 that the comment above that function derives; ordinary rows of this table keep
      |mean| / std <= RATIO_MAX = 2 (asserted in tests/test_pwdw_forms_cpu.py).  The zero and constant rows of the `special` cases have
      x - mean = 0 exactly, so an error of rstd multiplies nothing: what is left there is the rounding of mean . rstd, inside C_LN abar.
  depthwise   dy = sum_tap |w_tap| dt_tap + u_t |b| + 9 x 2^-11 S_y + 9 x 2^-25,   S_y = |b| + sum |w_tap t_tap|
      nine fp16 FMAs rounded to nearest (dw_row_f16: __builtin_elementwise_fma on fp16 pairs), each of relative error 2^-11 on a
      partial sum of at most S_y -- and of absolute error 2^-25 where that partial sum is subnormal (the same line: the FMA's result is
      an fp16 value; this is the one term the issue's formula lacks, and it is the format's, not a fit).  fp32s: 10 x 2^-24 S_y.
  outputs     bound = u_out |ref| + eta_out + 1.1 dy + 2^-20 |ref|      (1.1: SiLU's largest slope; 2^-20: the fast SiLU, as rows_cases)
      eta_out = 2^-25 where the output is stored as binary16 (a subnormal result is rounded to a multiple of 2^-24), else 0
      z: rows_cases' SILU_SPLIT bound, u_out |z| + 1.1 (c_mode S_t + S_pro) + 2^-20 |z|
      PROJ: dv = u_op |y| + eta_out + 1.1 dy (v is rounded to the stored type before the second 1x1: fd_pack_bf16), carried through
      |Weff| and |gate|: u_out |ref| + |gate| (c_mode(64) sum |Weff| |y| + sum |Weff| dv) + 2^-20 (|ref| + |x|), GATE_RES's residual term
  Gram partial of a workgroup that walked n_p pixels
      sum_p (|q| dk + |k| dq + dq dk) + (n_p + 8) 2^-24 sum_p |q k|,  dq = dk = 1.1 dy;  the norms: the same with i = j.
Saturation above 65504 is out of scope (it differs between the builds by design); range-hi scales the 1x1 output to a few thousand.

restate() is the same launch in fp32 torch with the kernels' rounding points (xn packed to the 16-bit type, the fp16 tile rounded toward
zero or to nearest, the fp16 FMA chain, the rounding of the stored output); tests/test_pwdw_forms_cpu.py checks error_bounds with it
before any kernel is asked: it passes on every case, and with one seeded fault each (a halo pixel taken from the clamped neighbour
instead of the zero padding, a channel pair swapped, a tile's second weight group taken from the first) it fails."""
from collections import namedtuple

import torch
import torch.nn.functional as F

import conv_cases as cc
import rows_cases as rc

ENTRIES = ("fd_pw_dw3x3", "fd_pw_dw3x3_proj", "fd_pw_dw3x3_gram", "fd_dwconv_gram", "fd_pw_dw3x3_f32", "fd_pw_dw3x3_gram_f32",
           "fd_pw_dw3x3_proj_f32")
DW, PROJ, GRAM, DWGRAM, F32, GRAM32, PROJ32 = ENTRIES
FP32S = (F32, GRAM32, PROJ32)
FD_F32, FD_BF16, LOW_LATENCY = 0, 1, 0x100
EPS = rc.EPS
ETA = 2.0 ** -24
RATIO_MAX = 2.0
# largest |xn32 - xn64| / abar over every case of this module, xn32 the prologue in fp32 torch (measure_c_ln, CPU): 4.1e-7 on bfloat16
# operands, 4.8e-7 on binary16, 2.14e-6 on fp32 operands (f32-96-b1-row and others without affine: an element with x and the row's mean
# both near zero, where the mean's own rounding is all that is left -- rows_cases.C_LN_MEASURED met the same); one constant: the largest
C_LN_MEASURED = 2.14e-6
C_LN = 4 * C_LN_MEASURED * (1 + RATIO_MAX ** 2)

# entry: a name of ENTRIES; cin, cdw, cz: fd_pw_dw3x3's (the other entries fix them); C: fd_dwconv_gram's; out_v: fd_pw_dw3x3_gram
# writes v; lowlat: FD_OPT_LOW_LATENCY; strided: every operand a slice of wider rows, ln_ld / gate_ld / ld_wdw above their packed
# values, shift / scale (/ gate) slots 3, 4 (, 5) of a 6 C row; special: zero and constant rows; rng: "", "hi" or "lo"; sparse: the last
# image is zero (and its shift is zero, so its LayerNorm'd rows and 1x1 output are exactly zero) but for SPARSE_PIXELS on the border and on
# tile corners -- a Gram partial sums over a workgroup's 512 to 1024 pixels, and a bound that sums every pixel's worst case cannot see
# three wrong pixels among them; on a sparse image the sums hold little else, so the padding rule shows in the partials too
PCase = namedtuple("PCase", "name entry B H W cin cdw cz C affine bias silu out_v lowlat strided special rng sparse")


def _p(name, entry, B, hw, cin=64, cdw=0, cz=0, C=0, affine=True, bias=True, silu=True, out_v=True, lowlat=False, strided=False,
       special=False, rng="", sparse=False):
    assert entry in ENTRIES and rng in ("", "hi", "lo") and not (sparse and affine and entry != DWGRAM)
    if entry in (PROJ, PROJ32):
        cdw, cz, bias, silu = 64, 0, False, False
    elif entry == GRAM:
        cdw, cz, bias, silu = 192, 0, False, False
    elif entry == GRAM32:
        cdw, cz, bias, silu = 128, 0, False, False
    elif entry == DWGRAM:
        cin, cdw, cz, bias, silu, affine = 0, 2 * C, 0, False, False, False
    if entry == F32:
        cz = 0
    return PCase(name, entry, B, hw[0], hw[1], cin, cdw, cz, C, affine, bias, silu, out_v, lowlat, strided, special, rng, sparse)


# 16-bit kernels, 8 x 16 tiles, >= 32768 px
ROW, COL = (8, 4096), (2048, 16)          # 256 tiles in one tile row / one tile column: every tile on two opposite borders
R3 = (136, 304)                           # 17 x 19 = 323 tiles: 323 % 4 = 3, 323 % 8 = 3
R1 = (264, 144)                           # 33 x 9 = 297 tiles: 297 % 4 = 1, 297 % 8 = 1 -- the last workgroup holds one tile
EX = (128, 256)                           # 256 tiles: exact
# fp32-storage kernels, 8 x 16 (DW) and 8 x 8 (GRAM, PROJ) tiles, >= 16384 px
SQ = (128, 128)                           # 128 tiles of 8 x 16 / 256 of 8 x 8: exact
ROW32 = (8, 2048)
COL16, COL8 = (1024, 16), (2048, 8)
R2_16 = (136, 160)                        # 17 x 10 = 170 tiles of 8 x 16: 170 % 4 = 2
R3_8 = (136, 152)                         # 17 x 19 = 323 tiles of 8 x 8: 323 % 16 = 3, 323 % 8 = 3, 323 % 2 = 1

CASES = [
    # ---- fd_pw_dw3x3, Cin = 64: pwdw_kernel<64>
    _p("dw64-128-128-b4-r3", DW, 4, R3, cdw=128, cz=128),
    _p("dw64-128-0-silu-b1", DW, 1, EX, cdw=128, cz=0),                                       # the z-recompute route
    _p("dw64-192-0-b4-exact", DW, 4, EX, cdw=192, affine=False, bias=False, silu=False),      # qkv + qkv_dwconv
    _p("dw64-64-0-b1-row", DW, 1, ROW, cdw=64, bias=False),
    _p("dw64-64-32-b4-r1", DW, 4, R1, cdw=64, cz=32, affine=False, silu=False),
    _p("dw64-128-96-b1-col", DW, 1, COL, cdw=128, cz=96),
    _p("dw64-strided", DW, 2, R1, cdw=128, cz=128, strided=True),
    _p("dw64-special", DW, 4, ROW, cdw=128, cz=128, special=True),
    _p("dw64-range-hi", DW, 1, EX, cdw=128, cz=128, rng="hi"),
    _p("dw64-range-lo", DW, 1, EX, cdw=128, cz=128, silu=False, rng="lo"),
    # ---- fd_pw_dw3x3, Cin = 128: pwdw_kernel<128>
    _p("dw128-256-256-b4-r3", DW, 4, R3, cin=128, cdw=256, cz=256),
    _p("dw128-256-0-b1", DW, 1, EX, cin=128, cdw=256, cz=0),
    _p("dw128-64-32-b4-exact", DW, 4, EX, cin=128, cdw=64, cz=32, affine=False, bias=False, silu=False),
    _p("dw128-192-64-b1-r1", DW, 1, R1, cin=128, cdw=192, cz=64, silu=False),
    _p("dw128-strided", DW, 1, ROW, cin=128, cdw=64, cz=32, strided=True),
    _p("dw128-special", DW, 1, COL, cin=128, cdw=256, cz=0, special=True),
    _p("dw128-range-hi", DW, 1, EX, cin=128, cdw=64, cz=32, rng="hi"),
    _p("dw128-range-lo", DW, 1, EX, cin=128, cdw=64, cz=32, silu=False, rng="lo"),
    # ---- fd_pw_dw3x3_proj: pwdw_kernel<64, PROJ>
    _p("proj-b1-exact", PROJ, 1, EX, affine=False),
    _p("proj-b4-r3", PROJ, 4, R3, affine=False),
    _p("proj-b4-row-affine", PROJ, 4, ROW),
    _p("proj-strided", PROJ, 1, COL, affine=False, strided=True),
    _p("proj-special", PROJ, 4, R1, affine=False, special=True),
    _p("proj-range-hi", PROJ, 1, EX, affine=False, rng="hi"),
    _p("proj-range-lo", PROJ, 1, EX, affine=False, rng="lo"),
    # ---- fd_pw_dw3x3_gram: pwdw_gram_kernel, 8 tiles per workgroup (4 under FD_OPT_LOW_LATENCY)
    _p("gram-v-exact", GRAM, 1, EX, affine=False),
    _p("gram-nov-r3", GRAM, 2, R3, affine=False, out_v=False),
    _p("gram-v-row-affine", GRAM, 1, ROW),
    _p("gram-nov-col", GRAM, 1, COL, affine=False, out_v=False),
    _p("gram-ll-v-r1", GRAM, 1, R1, affine=False, lowlat=True),
    _p("gram-ll-nov-exact", GRAM, 2, EX, affine=False, out_v=False, lowlat=True),
    _p("gram-strided", GRAM, 1, R1, affine=False, strided=True),
    _p("gram-special", GRAM, 2, ROW, affine=False, special=True),
    _p("gram-range-hi", GRAM, 1, EX, affine=False, rng="hi"),
    _p("gram-range-lo", GRAM, 1, EX, affine=False, rng="lo"),
    _p("gram-sparse", GRAM, 2, R1, affine=False, out_v=False, sparse=True),
    # ---- fd_dwconv_gram: dwconv_gram_kernel, 1 tile per workgroup below 64 tiles, 2 from 64, 4 from 256; ld > 3 C always
    _p("dwgram-1tile-c64", DWGRAM, 2, (8, 16), C=64),
    _p("dwgram-64t-c128", DWGRAM, 2, (64, 128), C=128),                  # the first shape with 2 tiles per workgroup
    _p("dwgram-63t-c64", DWGRAM, 1, (72, 112), C=64),                    # the last with 1
    _p("dwgram-63t-c320", DWGRAM, 1, (72, 112), C=320),                  # five head pairs
    _p("dwgram-256t-c128", DWGRAM, 1, EX, C=128),                        # the first with 4
    _p("dwgram-255t-c64", DWGRAM, 2, (136, 240), C=64),                  # 2 per workgroup, odd: the last holds one
    _p("dwgram-323t-c64", DWGRAM, 1, R3, C=64),                          # 4 per workgroup, the last holds three
    _p("dwgram-special", DWGRAM, 2, (64, 128), C=64, special=True),
    _p("dwgram-range-hi", DWGRAM, 1, (64, 128), C=64, rng="hi"),
    _p("dwgram-range-lo", DWGRAM, 1, (64, 128), C=64, rng="lo"),
    _p("dwgram-sparse", DWGRAM, 2, (64, 128), C=64, sparse=True),
    # ---- fd_pw_dw3x3_f32: pwdw32_kernel<DW, 16>
    _p("f32-32-b1", F32, 1, SQ, cdw=32, bias=False),
    _p("f32-64-b4-r2", F32, 4, R2_16, cdw=64),
    _p("f32-96-b1-row", F32, 1, ROW32, cdw=96, affine=False, silu=False),
    _p("f32-128-b4-exact", F32, 4, SQ, cdw=128),
    _p("f32-128-b1-col", F32, 1, COL16, cdw=128, bias=False, silu=False),
    _p("f32-strided", F32, 2, R2_16, cdw=96, strided=True),
    _p("f32-special", F32, 4, ROW32, cdw=64, special=True),
    # ---- fd_pw_dw3x3_gram_f32: pwdw32_kernel<GRAM, 8>, 16 tiles per workgroup
    _p("gram32-exact", GRAM32, 2, SQ, affine=False),
    _p("gram32-r3", GRAM32, 1, R3_8, affine=False),
    _p("gram32-row-affine", GRAM32, 1, ROW32),
    _p("gram32-col", GRAM32, 1, COL8, affine=False),
    _p("gram32-strided", GRAM32, 1, R3_8, affine=False, strided=True),
    _p("gram32-special", GRAM32, 2, COL8, affine=False, special=True),
    _p("gram32-sparse", GRAM32, 2, R3_8, affine=False, sparse=True),
    # ---- fd_pw_dw3x3_proj_f32: pwdw32_kernel<PROJ, 8>, 2 tiles per workgroup (8 from B = 4)
    _p("proj32-b1-exact", PROJ32, 1, SQ, affine=False),
    _p("proj32-b1-r3", PROJ32, 1, R3_8, affine=False),
    _p("proj32-b4-r3", PROJ32, 4, R3_8, affine=False),
    _p("proj32-b4-exact-affine", PROJ32, 4, SQ),
    _p("proj32-b1-col", PROJ32, 1, COL8, affine=False),
    _p("proj32-b2-row", PROJ32, 2, ROW32, affine=False),
    _p("proj32-strided", PROJ32, 2, R3_8, affine=False, strided=True),
    _p("proj32-special", PROJ32, 4, ROW32, affine=False, special=True),
]

# bit for bit.  Batch invariance: image 0 of the B = 4 launch against the same image alone (4 or 8 tiles per workgroup against 1 or 2);
# the Gram kernels: every image b of B = 4 against image b alone, partials included
BATCH_CASES = [
    _p("inv-dw64", DW, 4, R3, cdw=128, cz=128),
    _p("inv-dw128", DW, 4, R1, cin=128, cdw=256, cz=256),
    _p("inv-proj", PROJ, 4, R3, affine=False),
    _p("inv-gram", GRAM, 4, R1, affine=False),
    _p("inv-dwgram", DWGRAM, 4, (136, 240), C=128),
    _p("inv-f32", F32, 4, R2_16, cdw=128),
    _p("inv-gram32", GRAM32, 4, R3_8, affine=False),
    _p("inv-proj32", PROJ32, 4, R3_8, affine=False),
]
# across forms: the v of fd_pw_dw3x3_gram against the v third of fd_pw_dw3x3 at Cdw = 192; partials with and without out_v; v under
# FD_OPT_LOW_LATENCY; fd_pw_dw3x3_proj against the row-GEMM on the stored v (B = 1 and B = 4)
CROSS_CASES = [_p("cross-b1-r1", GRAM, 1, R1, affine=False), _p("cross-b4-r3", GRAM, 4, R3, affine=False)]
REPEAT = ("dw64-128-128-b4-r3", "dw128-256-256-b4-r3", "proj-b4-r3", "gram-nov-r3", "dwgram-323t-c64", "f32-64-b4-r2", "gram32-r3",
          "proj32-b4-r3")


def case_id(c):
    return c.name


def is32(c):
    return c.entry in FP32S


def npx(c):
    return c.H * c.W


def ndw(c):
    """depthwise channels of the launch (fd_pw_dw3x3_gram: q | k | v, computed whether or not v is stored)"""
    return c.cdw


Geo = namedtuple("Geo", "unit ld_x off_x ld_dw off_dw ld_z off_z ln_ld shift_off scale_off gate_ld gate_off ld_wdw ld_qkv")


def geom(c):
    """strides and offsets of the operands (elements).  Packed: rows as wide as their channels, shift | scale a [B, 2 Cin] row, the gate
    a row of its own.  Strided: slices of wider rows at non-zero offsets (multiples of 8; 4 in fp32 storage), and the modulation the
    engine's: slots 3, 4 (shift, scale) and 5 (gate) of a row of 6 Cin (+ 4 slack) floats"""
    u = 4 if is32(c) else 8
    nout = 64 if c.entry in (PROJ, PROJ32, GRAM) else c.cdw            # channels of the tensor stored through out_dw / out_v / out
    nw = c.cdw                          # tap columns; only the Gram / project_out forms of fp32 storage take a row stride for them
    if c.strided:
        return Geo(u, c.cin + 2 * u, u, nout + 3 * u, 2 * u, c.cz + 2 * u, u, 6 * c.cin + 4, 3 * c.cin, 4 * c.cin, 6 * c.cin + 4,
                   5 * c.cin, nw + (4 if c.entry in (GRAM32, PROJ32) else 0), 3 * c.C + 8)
    return Geo(u, c.cin, 0, nout, 0, c.cz, 0, 2 * c.cin, 0, c.cin, 64, 0, nw, 3 * c.C + 8)


def dtype_opts(c):
    return (FD_F32 if is32(c) else FD_BF16) | (LOW_LATENCY if c.lowlat else 0)


def plan(lib, c, B=None):
    """fd_pw_dw3x3_plan's answer for the case as a dict, None where the entry's _ok query refuses (host only)"""
    from founddiff_amd import _lib as L
    return L.pwdw_plan(lib, c.entry, dtype_opts(c), c.cin, c.cdw, c.cz, c.C, c.B if B is None else B, c.H, c.W)


# ------------------------------------------------------------------------------------------------ operands
# (image, y, x, value of every channel): image and tile corners, borders; negative indices count from the end
SPECIAL_PIXELS = ((0, 0, 0, 0.0), (0, 0, 5, 1.5), (-1, -1, -1, -0.75), (0, 7, 15, 0.0), (0, 7, 16, 1.5), (-1, -8, 0, 0.0),
                  (0, 3, -1, -0.75), (-1, -1, 8, 0.0))
# (y, x) of the live pixels of a sparse image: beside the image border, on tile corners, next to each other across a tile edge
SPARSE_PIXELS = ((0, 3), (5, 0), (7, 15), (7, 16), (8, 16), (2, -1), (-1, -2), (-8, 7), (-1, 0))
RANGE_SCALE = {"": 1.0, "hi": 2.0 ** 11, "lo": 2.0 ** -17}


def make_inputs(c, rq, seed=11):
    """the operands on the CPU in fp32, holding exactly the values the library will read: rq rounds what it stores in its 16-bit type
    (x, the 1x1 weights, Weff, qkv); the taps of the 16-bit kernels are rounded to fp16 (they are handed over as fp16 pairs); the 1x1
    weights of the fp32-storage kernels are hi + lo of their bf16 split (w_hi, w_lo)."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    ge, P, sc = geom(c), npx(c), RANGE_SCALE[c.rng]
    t = {}
    if c.entry == DWGRAM:
        # (the range cases scale q and k themselves: a few thousand / ~1e-5 with taps of O(1/3))
        t["qkv"] = rq(rn(c.B, P, ge.ld_qkv) * 0.7 * sc)
        t["taps"] = (rn(9, 3 * c.C) / 3).half().float()
        _special(c, t["qkv"].view(c.B, c.H, c.W, -1))
        _sparse(c, t["qkv"].view(c.B, c.H, c.W, -1))
        return t
    t["x"] = rq(rn(c.B, P, ge.ld_x) * 1.3 + 0.2)
    _special(c, t["x"].view(c.B, c.H, c.W, -1))
    t["ln_gamma"], t["ln_beta"] = 1 + 0.3 * rn(c.cin), 0.4 * rn(c.cin)
    t["ln_mod"] = 0.5 * rn(c.B, ge.ln_ld)
    if c.sparse:
        _sparse(c, t["x"].view(c.B, c.H, c.W, -1))
        t["ln_mod"][-1, ge.shift_off:ge.shift_off + c.cin] = 0
    w = rn(c.cdw + c.cz, c.cin) / c.cin ** 0.5 * sc
    if is32(c):
        hi = w.bfloat16().float()
        lo = (w - hi).bfloat16().float()
        t["w_hi"], t["w_lo"], t["w_pw"] = hi, lo, hi + lo
        t["taps"] = rn(9, ge.ld_wdw) / 3
    else:
        t["w_pw"] = rq(w)
        t["taps"] = (rn(9, c.cdw) / 3).half().float()
    if c.bias:
        t["b_dw"] = 0.5 * rn(c.cdw) * sc
    if c.entry in (PROJ, PROJ32):
        t["w2"] = rq(rn(c.B, 64, 64) / 8)
        if not c.strided:
            t["gate"] = 0.5 * rn(c.B, ge.gate_ld)
    return t


def _special(c, x4):
    if c.special:
        for b, y, x, v in SPECIAL_PIXELS:
            x4[b, y, x % c.W if x >= 0 else x] = v


def _sparse(c, x4):
    if c.sparse:
        live = [x4[-1, y, x % c.W if x >= 0 else x].clone() for y, x in SPARSE_PIXELS]
        x4[-1] = 0
        for (y, x), v in zip(SPARSE_PIXELS, live):
            x4[-1, y, x % c.W if x >= 0 else x] = v


def batch_slice(c, t, i):
    """(case, operands) of image i alone"""
    shared = {"ln_gamma", "ln_beta", "w_pw", "w_hi", "w_lo", "taps", "b_dw"}
    return c._replace(B=1), {k: (v if k in shared else v[i:i + 1].contiguous()) for k, v in t.items()}


def _pro_case(c):
    ge = geom(c)
    return rc._r(c.name, c.B, (c.H, c.W), c.cin, 32, ld0=ge.ld_x, off0=ge.off_x, pro="LN_MOD", affine=c.affine, ln_ld=2 * c.cin)


def _pro_operands(c, t):
    ge, m = geom(c), t["ln_mod"]
    return dict(in0=t["x"], ln_gamma=t["ln_gamma"], ln_beta=t["ln_beta"],
                ln_mod=torch.cat((m[:, ge.shift_off:ge.shift_off + c.cin], m[:, ge.scale_off:ge.scale_off + c.cin]), 1))


def gate_of(c, t):
    ge = geom(c)
    return (t["ln_mod"] if c.strided else t["gate"])[:, ge.gate_off:ge.gate_off + 64]


def taps_of(c, t):
    return t["taps"][:, :ndw(c)] if c.entry != DWGRAM else t["taps"][:, :2 * c.C]


def row_ratio(c, t):
    """largest |mean| / std over the ordinary rows of x (rows of zero variance, the special ones, left out)"""
    x = t["x"].view(c.B, npx(c), -1)[..., geom(c).off_x:geom(c).off_x + c.cin].double()
    sd = x.std(-1, unbiased=False)
    return float((x.mean(-1).abs() / sd)[sd > 0].max())


def measure_c_ln(c, rq, dev="cpu"):
    """largest |xn32 - xn64| / abar of one case: the prologue in fp32 torch against fp64"""
    t = _pro_operands(c, make_inputs(c, rq))
    p64, p32 = rc.prologue(_pro_case(c), t, torch.float64, dev), rc.prologue(_pro_case(c), t, torch.float32, dev)
    return worst((p32["a"].double() - p64["a"]).abs(), p64["abar"])[0]          # (abar = 0, the dead rows of a sparse image: exact)


# ------------------------------------------------------------------------------------------------ the reference
def dw3x3(t4, w9):
    """sum_tap w9[3 dy + dx] t4[y + dy - 1, x + dx - 1] on [B, H, W, C] with zero padding (cross-correlation, as nn.Conv2d)"""
    H, W = t4.shape[1:3]
    pad = F.pad(t4, (0, 0, 1, 1, 1, 1))
    out = torch.zeros_like(t4)
    for dy in range(3):
        for dx in range(3):
            out += pad[:, dy:dy + H, dx:dx + W] * w9[3 * dy + dx]
    return out


def unit_roundoffs(c, tdt):
    """(u_t of the on-chip 1x1 tile, eta, u_h of the packed xn = u_op of the stored v, eta_out of a stored output, the depthwise
    accumulation's relative and absolute term)"""
    if is32(c):
        return 0.0, 0.0, 0.0, 0.0, 10 * 2.0 ** -24, 0.0
    fp16 = tdt == torch.float16
    return (2.0 ** -11 if fp16 else 2.0 ** -10), ETA, cc.U_OUT[tdt], (2.0 ** -25 if fp16 else 0.0), 9 * 2.0 ** -11, 9 * 2.0 ** -25


def pwdw_reference(c, t, tdt, dev):
    """The launch restated in fp64 on `dev` -> dict of fp64 tensors: y [B, H, W, ndw] the depthwise output before SiLU with dy, its
    error's bound ahead of the output's own rounding (module docstring); z / z_pre (the bound of z ahead of its rounding) [B, H, W, Cz];
    x (the block input's own channels) for the PROJ forms.  tdt: the stored element type."""
    f64 = torch.float64
    D = lambda k: t[k].to(dev, f64)
    u_t, eta, u_h, _, acc_rel, acc_abs = unit_roundoffs(c, tdt)
    mode = "fp32s" if is32(c) else "bf16"
    n, r = ndw(c), {}
    w9 = taps_of(c, t).to(dev, f64)
    if c.entry == DWGRAM:
        tt = D("qkv").view(c.B, c.H, c.W, -1)[..., :2 * c.C]
        dt = torch.full_like(tt, eta)
    else:
        pr = rc.prologue(_pro_case(c), _pro_operands(c, t), f64, dev)
        a, w = pr["a"], D("w_pw")
        tt, S_t = a @ w.T, a.abs() @ w.abs().T
        S_pro = (u_h * a.abs() + C_LN * pr["abar"]) @ w.abs().T
        cS = rc.c_mode(c.cin, mode) * S_t + S_pro
        dt = (u_t * tt.abs() + eta + cS)[..., :n].reshape(c.B, c.H, c.W, n)
        if c.cz:
            zp = tt[..., n:]
            r["z"] = (zp * torch.sigmoid(zp)).reshape(c.B, c.H, c.W, c.cz)
            r["z_pre"] = (1.1 * cS[..., n:]).reshape(c.B, c.H, c.W, c.cz)
        r["x"] = rc._sources(_pro_case(c), _pro_operands(c, t), f64, dev).reshape(c.B, c.H, c.W, c.cin)
        tt = tt[..., :n].reshape(c.B, c.H, c.W, n)
        del pr, a, S_t, S_pro, cS
    b = D("b_dw") if c.bias else torch.zeros(n, dtype=f64, device=dev)
    r["y"] = dw3x3(tt, w9) + b
    S_y = dw3x3(tt.abs(), w9.abs()) + b.abs()
    r["dy"] = dw3x3(dt, w9.abs()) + u_t * b.abs() + acc_rel * S_y + acc_abs
    return r


def _tiles(v, TW):
    """[B, H, W, C] -> [B, tiles (row-major), 8 TW pixels, C]"""
    B, H, W, Cn = v.shape
    return v.view(B, H // 8, 8, W // TW, TW, Cn).permute(0, 1, 3, 2, 4, 5).reshape(B, (H // 8) * (W // TW), 8 * TW, Cn)


def _per_workgroup(v, pl):
    """[B, tiles, ...] -> [B, gx, ...]: the sum over each workgroup's own tiles, gx * tpw .. min(ntiles, (gx + 1) * tpw)"""
    B, nt = v.shape[:2]
    assert nt == pl["ntiles"] and pl["gx"] == -(-nt // pl["tpw"])
    full = torch.zeros((B, pl["gx"] * pl["tpw"]) + v.shape[2:], dtype=v.dtype, device=v.device)
    full[:, :nt] = v
    return full.view((B, pl["gx"], pl["tpw"]) + v.shape[2:]).sum(2)


def gram_slices(c):
    """(q channels, k channels, heads) of the depthwise output"""
    h = c.C if c.entry == DWGRAM else 64
    return slice(0, h), slice(h, 2 * h), h // 32


def gram_partials(c, y, dy, pl):
    """(reference, bound) of the partial buffer [B, heads, gx, 1024 + 64] from the depthwise output y [B, H, W, >= 2 h] and its error
    bound dy: per workgroup the Gram q k^T (rows = q channels) of each head, sum q^2, sum k^2 over the workgroup's own tiles"""
    qs, ks, heads = gram_slices(c)
    TW = pl["TW"]
    hd = lambda v, s: _tiles(v[..., s], TW).unflatten(-1, (heads, 32)).permute(0, 1, 3, 4, 2)       # [B, tiles, heads, 32, pixels]
    q, k, dq, dk = hd(y, qs), hd(y, ks), 1.1 * hd(dy, qs), 1.1 * hd(dy, ks)
    T = lambda v: v.transpose(-1, -2)
    wg = lambda v: _per_workgroup(v, pl).transpose(1, 2)                                             # -> [B, heads, gx, ...]
    n_p = torch.full((pl["gx"],), pl["tpw"] * 8 * TW, dtype=y.dtype, device=y.device)
    n_p[-1] = (pl["ntiles"] - (pl["gx"] - 1) * pl["tpw"]) * 8 * TW
    cacc = ((n_p + 8) * 2.0 ** -24).view(1, 1, -1, 1)
    G = wg(q @ T(k)).flatten(-2)
    Gb = wg(q.abs() @ T(dk) + dq @ T(k.abs()) + dq @ T(dk)).flatten(-2) + cacc * wg(q.abs() @ T(k.abs())).flatten(-2)
    nq, nk = wg((q * q).sum(-1)), wg((k * k).sum(-1))
    nqb = wg((2 * q.abs() * dq + dq * dq).sum(-1)) + cacc * nq
    nkb = wg((2 * k.abs() * dk + dk * dk).sum(-1)) + cacc * nk
    return torch.cat((G, nq, nk), -1), torch.cat((Gb, nqb, nkb), -1)


def error_bounds(c, t, ref, tdt, pl, dev):
    """{output name: (reference, bound)} of everything the launch stores: out_dw [B, H, W, Cdw], z, v [B, H, W, 64] (fd_pw_dw3x3_gram
    with out_v), out (the PROJ forms), part [B, heads, gx, 1088].  From the inputs alone (module docstring)."""
    _, _, u_op, eta_out, _, _ = unit_roundoffs(c, tdt)
    u_out = cc.U_OUT[torch.float32 if is32(c) else tdt]
    y, dy = ref["y"], ref["dy"]
    stored = lambda v, pre: u_out * v.abs() + eta_out + pre + 2.0 ** -20 * v.abs()
    r = {}
    if c.entry in (DW, F32):
        o = y * torch.sigmoid(y) if c.silu else y
        r["out_dw"] = (o, stored(o, 1.1 * dy))
        if c.cz:
            r["z"] = (ref["z"], stored(ref["z"], ref["z_pre"]))
    elif c.entry in (PROJ, PROJ32):
        f64 = torch.float64
        w2 = t["w2"].to(dev, f64)                                         # [B, 64 out, 64 in]
        gate = gate_of(c, t).to(dev, f64)[:, None, None]
        lin = lambda v, m: (v.flatten(1, 2) @ m.transpose(1, 2)).view(v.shape)
        dv = u_op * y.abs() + eta_out + 1.1 * dy
        o = ref["x"] + gate * lin(y, w2)
        pre = gate.abs() * (rc.c_mode(64, "fp32s" if is32(c) else "bf16") * lin(y.abs(), w2.abs()) + lin(dv, w2.abs()))
        r["out"] = (o, u_out * o.abs() + eta_out + pre + 2.0 ** -20 * (o.abs() + ref["x"].abs()))
    else:
        r["part"] = gram_partials(c, y, dy, pl)
        if c.entry == GRAM and c.out_v:
            v = y[..., 128:]
            r["v"] = (v, stored(v, 1.1 * dy[..., 128:]))
    return r


# ------------------------------------------------------------------------------------------------ the fp32 restatement (CPU self-check)
def f16_rtz(v):
    """fp32 -> fp16 rounded toward zero, saturating (v_cvt_pkrtz_f16_f32), as an fp16 tensor"""
    h = v.to(torch.float16)
    away = h.float().abs() > v.abs()
    bits = h.view(torch.int16).to(torch.int32) & 0xFFFF
    bits = torch.where(away, bits - 1, bits)
    return torch.where(bits >= 32768, bits - 65536, bits).to(torch.int16).view(torch.float16)


FAULTS = ("clamped-halo", "swapped-pair", "previous-group")
# every fault sits in tile 0 of the LAST image (the sparse one, where the case has one): the halo pixel (-1, 3) above the live pixel
# (0, 3); the swapped pair is the last two depthwise channels where they are stored (the v of fd_pw_dw3x3_gram), else the first two


def restate(c, t, tdt, pl, fault=None):
    """The launch in fp32 torch on the CPU with the kernels' rounding points -> {output name: tensor as stored}.  fault: one of FAULTS,
    a wrong result of the size a broken kernel would give (in one tile)."""
    f32 = torch.float32
    fp16b = tdt == torch.float16
    to_tile = (lambda v: v) if is32(c) else ((lambda v: v.to(torch.float16)) if fp16b else f16_rtz)
    rq = (lambda v: v) if is32(c) else (lambda v: v.to(tdt).float())
    n, TW = ndw(c), pl["TW"]
    w9 = taps_of(c, t)
    if c.entry == DWGRAM:
        tile = to_tile(t["qkv"].view(c.B, c.H, c.W, -1)[..., :2 * c.C])
    else:
        pt = _pro_operands(c, t)
        a = rc.prologue(_pro_case(c), pt, f32, "cpu")["a"]
        if is32(c):
            ah = a.bfloat16().float()
            al = (a - ah).bfloat16().float()
            tt = al @ t["w_hi"].T + ah @ t["w_lo"].T + ah @ t["w_hi"].T
        else:
            tt = rq(a) @ t["w_pw"].T
        tt = tt.view(c.B, c.H, c.W, -1)
        if fault == "previous-group":
            assert n >= 64
            tt[-1, :8, :TW, 32:64] = tt[-1, :8, :TW, 0:32]
        tile = to_tile(tt[..., :n])
        zpre = tt[..., n:]
    if fault == "swapped-pair":
        pair = [n - 2, n - 1] if c.entry == GRAM and c.out_v else [0, 1]
        tile[-1, :8, :TW, pair] = tile[-1, :8, :TW, pair[::-1]]
    pad = F.pad(tile, (0, 0, 1, 1, 1, 1))
    if fault == "clamped-halo":
        pad[-1, 0, 4] = tile[-1, 0, 3]             # halo pixel (-1, 3) of tile 0 from its clamped neighbour (0, 3)
    if is32(c):
        acc = (t["b_dw"] if c.bias else torch.zeros(n)).expand(c.B, c.H, c.W, n).clone()
        for k in range(9):
            acc += w9[k] * pad[:, k // 3:k // 3 + c.H, k % 3:k % 3 + c.W]
        y = acc
    else:
        acc = to_tile(t["b_dw"] if c.bias else torch.zeros(n)).expand(c.B, c.H, c.W, n)
        for k in range(9):                             # fp16 FMA: the exact product and sum, rounded once to fp16
            acc = (pad[:, k // 3:k // 3 + c.H, k % 3:k % 3 + c.W].double() * w9[k].double() + acc.double()).to(torch.float16)
        y = acc.float()
    r = {}
    if c.entry in (DW, F32):
        r["out_dw"] = rq(F.silu(y) if c.silu else y)
        if c.cz:
            r["z"] = rq(F.silu(zpre))
    elif c.entry in (PROJ, PROJ32):
        x = rc._sources(_pro_case(c), pt, f32, "cpu").view(c.B, c.H, c.W, -1)
        if is32(c):
            vh = y.bfloat16().float()
            vl = (y - vh).bfloat16().float()
            wh = t["w2"].bfloat16().float()
            wl = (t["w2"] - wh).bfloat16().float()
            lin = lambda v, m: (v.flatten(1, 2) @ m.transpose(1, 2)).view(v.shape)
            val = lin(vh, wl) + lin(vl, wh) + lin(vh, wh)
        else:
            val = (rq(y).flatten(1, 2) @ t["w2"].transpose(1, 2)).view(y.shape)
        r["out"] = rq(x + gate_of(c, t)[:, None, None] * val)
    else:
        qs, ks, heads = gram_slices(c)
        hd = lambda s: _tiles(y[..., s], TW).unflatten(-1, (heads, 32)).permute(0, 1, 3, 4, 2)
        q, k = hd(qs), hd(ks)
        wg = lambda v: _per_workgroup(v, pl).transpose(1, 2)
        r["part"] = torch.cat((wg(q @ k.transpose(-1, -2)).flatten(-2), wg((q * q).sum(-1)), wg((k * k).sum(-1))), -1)
        if c.entry == GRAM and c.out_v:
            r["v"] = rq(y[..., 128:])
    return r


def worst(err, bound):
    """largest err / bound and its index; a bound of exactly 0 admits err = 0 only"""
    bound = bound.expand_as(err)
    ratio = torch.where(bound > 0, err / bound, torch.where(err > 0, float("inf"), 0.0).to(err.dtype))
    i = int(ratio.argmax())
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ratio.shape))
    return float(ratio.flatten()[i]), idx, float(err[idx]), float(bound[idx])


def where_in_tile(idx, TW):
    """(image, y, x, channel) -> 'tile n (ty, tx), row r, column s of the tile'"""
    _, y, x = idx[:3]
    return f"tile (row {y // 8}, column {x // TW}), position (row {y % 8}, column {x % TW}) of the tile"
