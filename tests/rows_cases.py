"""The shapes of tests/test_gpu_rows_forms.py, and the fp64 restatement of the streaming row-GEMM they are compared with.

fd_conv_kernel_id 10 (csrc/fd_gemm_rows.hip, 16-bit storage) and 17 (csrc/fd_gemm_rows32.hip, fp32 storage, split-bf16 contraction) are
gemm_rows_kernel<KS, PRO, EPI, NT> / gemm_rows32_kernel<KS, PRO, EPI, NT> in 169 + 120 compiled forms, and four z-recompute kernels.
Which one a launch runs, on which grid, is fd_gemm_rows_form's answer (host only).  rows_cases() holds
  * one generated case per form the plan can reach: for every (mode, K, prologue, epilogue) the output widths at which the plan's own
    answer says NT 256 (the widest such: the last weight image before the workgroup grows), 512 and 768 (the narrowest), found by
    asking the query, not by a copy of its LDS arithmetic;
  * hand-written edge cases (EDGE_CASES) and tile-walk cases (WALK_CASES);
tests/test_rows_forms_cpu.py asserts from the query alone that they reach what its literal lists name.
gemm_rows_zre_kernel<4, 256, false> (the z-recompute kernel without its prefetch) is launched only under a development switch, which the
tested (release) build compiles to a constant: it is unreachable there and has no case."""
from collections import namedtuple

import torch

import conv_cases as cc

EPIS = cc.EPIS + ("GNSILU_ADD_FINAL",)             # value = index (include/founddiff_hip.h)
PROS = ("NONE", "LN_MOD", "LN_GATE", "ZRE")          # FD_PRO_*; ZRE = FD_PRO_LN_GATE_ZRE
MODES = ("bf16", "fp32s")                            # 'bf16': the build's 16-bit type (kernel id 10); 'fp32s': kernel id 17
KID = {"bf16": 10, "fp32s": 17}
PAIRS = [("NONE", e) for e in EPIS] + [("LN_MOD", "NONE"), ("LN_MOD", "SILU_SPLIT"), ("LN_GATE", "GATE_RES")]
KS_ALL = (1, 2, 3, 4, 6, 8)
EPS = 1e-5
FIN_B, FIN_ALPHA = 0.125, 0.37

# pro: a name of PROS; affine: the LayerNorm of LN_MOD (norm1 of ZRE) has gamma / beta; ln_ld: row stride of the per-image vectors
# (shift | scale of LN_MOD and of ZRE's norm1, `local` of LN_GATE / ZRE); ldz / offz: the z operand of LN_GATE; fin_mode / fin_last:
# GNSILU_ADD_FINAL; special: a few rows of zeros and of one constant value (zero variance) in the LayerNorm's operand
RCase = namedtuple("RCase", "name B H W cin c1 ld0 off0 ld1 off1 cout ldo offo bias wb epi split groups gate_ld ld_res off_res pro affine "
                            "ln_ld ldz offz fin_mode fin_last special modes")


def _r(name, B, hw, cin, cout, c1=0, ld0=None, off0=0, ld1=None, off1=0, ldo=None, offo=0, bias=True, wb=False, epi="NONE", split=0,
       groups=0, gate_ld=None, ld_res=None, off_res=0, pro="NONE", affine=True, ln_ld=None, ldz=None, offz=0, fin_mode=0, fin_last=0,
       special=False, modes=MODES):
    assert epi in EPIS and pro in PROS
    if pro == "ZRE":
        assert epi == "GATE_RES" and cin == 2 * cout and not wb and c1 == 0
    if epi in ("GNSILU_ADD", "GNSILU_ADD_FINAL"):
        groups = groups or 4
    return RCase(name, B, hw[0], hw[1], cin, c1, ld0 or cin - c1, off0, ld1 or c1, off1, cout, ldo or cout, offo, bias, wb, epi, split,
                 groups, gate_ld or cout, ld_res or cout, off_res, pro, affine, ln_ld or 2 * cin, ldz or cin, offz, fin_mode, fin_last,
                 special, tuple(modes))


TALL, TALL_E = cc.TALL, cc.TALL_E          # 16510 px (% 32 = 30, % 16 = 14) and 16402 px (% 32 = 18, % 16 = 2)
EXACT = (128, 128)                         # 16384 px: every tile full
ONE_ROW = (145, 113)                       # 16385 px: the last tile holds one row (and the second subtile of S = 2 is empty)
HALF = (100, 164)                          # 16400 px: % 32 = 16 -- S = 2: the last tile's first subtile full, its second empty
WALK2 = (181, 182)                         # 32942 px: at B = 4 the S = 2 kernels walk more than one tile per wave

H16 = ("bf16",)
EDGE_CASES = [
    # the c0 boundary inside a 32-channel MFMA step (40 + 24), both sources slices of wider rows
    _r("cat-40+24", 1, TALL, 64, 64, c1=24, ld0=48, off0=8, ld1=40, off1=16),
    _r("cat-72+56-relu", 1, TALL, 128, 32, c1=56, ld0=80, off0=8, ld1=64, off1=8, epi="RELU"),
    # SiLU from a channel that is no multiple of 32
    _r("silu-split-40", 1, TALL, 64, 96, epi="SILU_SPLIT", split=40),
    _r("silu-split-72-k96", 1, TALL, 96, 128, epi="SILU_SPLIT", split=72),
    # GroupNorm groups of 8 channels: a 32-column step spans four groups
    _r("gn-groups-of-8", 1, TALL, 64, 64, epi="GNSILU_ADD", groups=8),
    _r("gn-groups-of-8-k128", 1, TALL, 128, 96, epi="GNSILU_ADD", groups=12),
    # LN_MOD without affine, zero-variance rows
    _r("lnmod-noaffine", 1, TALL, 64, 64, pro="LN_MOD", affine=False, special=True),
    _r("lnmod-noaffine-k96-silu", 1, TALL, 96, 64, pro="LN_MOD", affine=False, epi="SILU_SPLIT", split=24, special=True),
    _r("lnmod-special-k128", 2, EXACT, 128, 64, pro="LN_MOD", special=True, ln_ld=2 * 128 + 12),
    # every stride at once: z, gate, residual, output and input all slices of wider rows
    _r("lngate-all-strided", 2, TALL, 128, 64, ld0=136, off0=8, ldo=80, offo=8, epi="GATE_RES", gate_ld=76, ld_res=72, off_res=8,
       pro="LN_GATE", ln_ld=128 + 4, ldz=264, offz=136, special=True),
    _r("lngate-special-k64", 1, ONE_ROW, 64, 32, epi="GATE_RES", pro="LN_GATE", ldz=128, offz=64, special=True),
    # per-image weights together with a prologue
    _r("wbatch-lnmod", 2, TALL, 64, 64, bias=False, wb=True, pro="LN_MOD"),
    _r("wbatch-lngate", 2, TALL, 96, 32, bias=False, wb=True, epi="GATE_RES", pro="LN_GATE"),
    _r("wbatch-gate-slice", 2, TALL, 64, 64, ld0=192, off0=128, bias=False, wb=True, epi="GATE_RES", gate_ld=384),
    # the final 1x1 and the sampler's update
    _r("final-mode0", 1, TALL, 64, 64, epi="GNSILU_ADD_FINAL", groups=8),
    _r("final-ddim", 2, TALL, 192, 64, c1=64, epi="GNSILU_ADD_FINAL", groups=8, fin_mode=1, fin_last=0),
    _r("final-ddim-last", 2, ONE_ROW, 128, 64, c1=64, epi="GNSILU_ADD_FINAL", groups=8, fin_mode=1, fin_last=1),
    _r("final-ddim-k32", 1, HALF, 32, 32, epi="GNSILU_ADD_FINAL", fin_mode=1, fin_last=0),
    # pixel-count edges, S = 2 (K <= 64 in 16 bits; the fp32s kernel runs the same cases with S = 1) and S = 1
    _r("s2-exact", 1, EXACT, 32, 32),                           # ... and Cout 32, the smallest
    _r("s2-one-row", 1, ONE_ROW, 64, 64, epi="RES_RELU", ld_res=72, off_res=8),
    _r("s2-half", 1, HALF, 64, 64, epi="GATE_RES"),
    _r("s2-half-lnmod", 1, HALF, 32, 64, pro="LN_MOD"),
    _r("s2-ragged-e", 1, TALL_E, 64, 32, ldo=48, offo=8),
    _r("s1-exact", 1, EXACT, 128, 64),
    _r("s1-one-row", 1, ONE_ROW, 96, 64, epi="RES_RELU"),
    _r("s1-ragged-e-k256", 1, TALL_E, 256, 32, epi="GATE_RES"),
    _r("s1-one-row-lngate-k192", 1, ONE_ROW, 192, 64, epi="GATE_RES", pro="LN_GATE", modes=MODES),
    # the z-recompute kernels: ragged and exact, with and without norm1's affine, strided, zero-variance rows of x and of y
    _r("zre128-ragged", 1, TALL, 128, 64, epi="GATE_RES", pro="ZRE"),
    _r("zre128-exact-special", 1, EXACT, 128, 64, epi="GATE_RES", pro="ZRE", special=True),
    _r("zre128-one-row-noaffine-strided", 2, ONE_ROW, 128, 64, ld0=136, off0=8, ldo=72, offo=8, epi="GATE_RES", gate_ld=68, ld_res=72,
       off_res=8, pro="ZRE", affine=False, ln_ld=2 * 128 + 4, bias=False),
    _r("zre256-ragged", 1, TALL, 256, 128, epi="GATE_RES", pro="ZRE", modes=H16),
    _r("zre256-exact-special", 1, EXACT, 256, 128, epi="GATE_RES", pro="ZRE", special=True, modes=H16),
    _r("zre256-one-row-noaffine-strided", 2, ONE_ROW, 256, 128, ld0=264, off0=8, ldo=136, offo=8, epi="GATE_RES", gate_ld=132,
       ld_res=136, off_res=8, pro="ZRE", affine=False, bias=False, modes=H16),
]

# the persistent tile walk: each family once with a wave per tile (grid x = need) and once with waves that walk >= 2 tiles and a
# ragged last round (wtiles no multiple of grid x . NT / 64) -- B = 4, which also moves the workgroups-per-CU limit from 4 to 3
WALK_CASES = [
    _r("walk-s2-one", 1, WALK2, 64, 64, epi="GATE_RES", modes=H16),
    _r("walk-s2-many", 4, WALK2, 64, 64, epi="GATE_RES", modes=H16),
    _r("walk-s2-many-lnmod", 4, WALK2, 64, 128, pro="LN_MOD", epi="SILU_SPLIT", split=64, modes=H16),
    _r("walk-s1-256-one", 1, TALL, 128, 64),
    _r("walk-s1-256-many", 4, TALL, 128, 64),
    _r("walk-s1-512-one", 1, TALL, 128, 256, epi="RELU", modes=H16),
    _r("walk-s1-512-many", 4, TALL, 128, 256, epi="RELU", modes=H16),
    _r("walk-s1-768-one", 1, TALL, 128, 320, pro="LN_MOD", modes=H16),
    _r("walk-s1-768-many", 4, TALL, 128, 320, pro="LN_MOD", modes=H16),
    _r("walk-zre128-many", 4, TALL, 128, 64, epi="GATE_RES", pro="ZRE"),
    _r("walk-zre256-many", 4, TALL, 256, 128, epi="GATE_RES", pro="ZRE", modes=H16),
    _r("walk-rows32-512-one", 1, TALL, 128, 160, epi="RES_RELU", modes=("fp32s",)),
    _r("walk-rows32-512-many", 4, TALL, 128, 160, epi="RES_RELU", modes=("fp32s",)),
]
# family -> (one tile per wave, several tiles per wave); (case name, mode)
WALK_FAMILIES = {
    "generic S=2": (("walk-s2-one", "bf16"), ("walk-s2-many", "bf16")),
    "generic S=1 NT 256": (("walk-s1-256-one", "bf16"), ("walk-s1-256-many", "bf16")),
    "generic S=1 NT 512": (("walk-s1-512-one", "bf16"), ("walk-s1-512-many", "bf16")),
    "generic S=1 NT 768": (("walk-s1-768-one", "bf16"), ("walk-s1-768-many", "bf16")),
    "zre K=128": (("zre128-ragged", "bf16"), ("walk-zre128-many", "bf16")),
    "zre K=256": (("zre256-ragged", "bf16"), ("walk-zre256-many", "bf16")),
    "rows32 NT 256": (("walk-s1-256-one", "fp32s"), ("walk-s1-256-many", "fp32s")),
    "rows32 NT 512": (("walk-rows32-512-one", "fp32s"), ("walk-rows32-512-many", "fp32s")),
    "rows32 zre": (("zre128-ragged", "fp32s"), ("walk-zre128-many", "fp32s")),
}

# bit-for-bit checks.  Batch invariance: image 0 of the B = 4 launch against the same image alone
BATCH_CASES = [
    _r("inv-none", 4, WALK2, 64, 64, bias=False),
    _r("inv-gate", 4, TALL, 128, 64, epi="GATE_RES"),
    _r("inv-lnmod-silu", 4, WALK2, 64, 128, pro="LN_MOD", epi="SILU_SPLIT", split=64),
    _r("inv-lngate", 4, TALL, 128, 64, epi="GATE_RES", pro="LN_GATE", ldz=256, offz=128),
    _r("inv-zre128", 4, TALL, 128, 64, epi="GATE_RES", pro="ZRE"),
    _r("inv-zre256", 4, TALL, 256, 128, epi="GATE_RES", pro="ZRE", modes=H16),
]
# column invariance (16-bit): (case whose Cout puts it on NT 512 / 768, that NT); its first 64 channels against a Cout = 64 launch
COLUMN_CASES = [(_r(f"col-{tag}-{nt}", 2, TALL, 128, co, modes=H16, **kw), nt)
                for co, nt in ((256, 512), (320, 768))
                for tag, kw in (("none", {}), ("gate", dict(epi="GATE_RES")), ("lnmod", dict(pro="LN_MOD")))]
# ... and fp32s: the whole launch against DAEngine.conv_cols chunks (in_proj 128 -> 256 in halves, bias-free)
COLS32_CASE = _r("cols32-lnmod-silu", 2, TALL, 128, 128, bias=False, pro="LN_MOD", epi="SILU_SPLIT", split=64, modes=("fp32s",))


def case_id(c):
    return c.name


def npx(c):
    return c.H * c.W


def conv_case(c):
    """the conv_cases.Case that carries the fields the two tables share (the final form as its GNSILU_ADD)"""
    return cc._c(c.name, c.B, (c.H, c.W), c.cin, c.cout, c1=c.c1, ld0=c.ld0, off0=c.off0, ld1=c.ld1, off1=c.off1, ldo=c.ldo, offo=c.offo,
                 bias=c.bias, wb=c.wb, epi="GNSILU_ADD" if c.epi == "GNSILU_ADD_FINAL" else c.epi, split=c.split, groups=c.groups,
                 gate_ld=c.gate_ld, ld_res=c.ld_res, off_res=c.off_res, modes=c.modes, kid=10, pw=0)


def cx_of(c):
    return c.cin // 2          # the width of the block input the z-recompute kernels read: d_inner = 2 dim


def params_for(c, mode, ptrs):
    """fd_conv_params of (case, mode): conv_cases.params_for, plus the prologue, fin_* and zre_* fields.  ptrs: as there, and ln_gamma,
    ln_beta, ln_mod, z, zre_w, zre_gamma, zre_beta, zre_mod, fin_w, fin_out, fin_img, fin_xin"""
    p = cc.params_for(conv_case(c), "bf16" if mode == "bf16" else "fp32s", ptrs)
    K = c.cin
    p.prologue, p.ln_eps, p.ln_ld = PROS.index(c.pro), EPS, c.ln_ld
    if c.pro == "LN_MOD":
        if c.affine:
            p.ln_gamma, p.ln_beta = ptrs["ln_gamma"], ptrs["ln_beta"]
        p.ln_shift, p.ln_scale = ptrs["ln_mod"], ptrs["ln_mod"] + 4 * K
    elif c.pro in ("LN_GATE", "ZRE"):
        p.ln_gamma, p.ln_beta, p.ln_shift = ptrs["ln_gamma"], ptrs["ln_beta"], ptrs["ln_mod"]
    if c.pro == "LN_GATE":
        p.ln_z, p.ln_ldz, p.ln_offz = ptrs["z"], c.ldz, c.offz
    if c.pro == "ZRE":
        CX = cx_of(c)
        p.zre_w, p.zre_shift, p.zre_scale, p.zre_ld, p.zre_eps = ptrs["zre_w"], ptrs["zre_mod"], ptrs["zre_mod"] + 4 * CX, c.ln_ld, EPS
        if c.affine:
            p.zre_gamma, p.zre_beta = ptrs["zre_gamma"], ptrs["zre_beta"]
    if c.epi == "GNSILU_ADD_FINAL":
        p.epilogue = EPIS.index(c.epi)
        p.fin_w, p.fin_b, p.fin_out, p.fin_mode, p.fin_last = ptrs["fin_w"], FIN_B, ptrs["fin_out"], c.fin_mode, c.fin_last
        if c.fin_mode:
            p.fin_img, p.fin_xin, p.fin_alpha = ptrs["fin_img"], ptrs["fin_xin"], FIN_ALPHA
    return p


_NAMES = ("in0 in1 weight bias out res gate h gn gamma beta stats ln_gamma ln_beta ln_mod z zre_w zre_gamma zre_beta zre_mod fin_w fin_out "
          "fin_img fin_xin").split()
DUMMY_PTRS = {n: 0x100000 * (i + 1) for i, n in enumerate(_NAMES)}


def form(lib, c, mode, ptrs=None):
    """fd_gemm_rows_form's answer for (case, mode) as a dict, None when the case does not run on the row-GEMM"""
    from founddiff_amd import _lib as L
    return L.rows_form(lib, params_for(c, mode, ptrs or DUMMY_PTRS))


def kernel_of(f):
    """the compiled kernel a plan names: ('zre', n) or (KS, PRO, EPI, NT) with the template's PRO / EPI"""
    if f["zre"]:
        return ("zre", f["zre"])
    pro = PROS[f["PRO"]]
    epi = EPIS[f["EPI"]]
    if pro == "LN_MOD" and epi != "SILU_SPLIT":
        epi = "NONE"
    return (f["KS"], pro, epi, f["NT"])


# ------------------------------------------------------------------------------------------------ generated cases
COUT_STEP, COUT_MAX = 32, 1024


def generated_cases(lib):
    """one case per (mode, K, prologue, epilogue, NT) the plan reaches at B = 1: the Cout comes from the query's own answers"""
    out = []
    for mode in MODES:
        for KS in KS_ALL:
            for pro, epi in PAIRS:
                mk = lambda co, nt=0: _r(f"g-{mode}-k{32 * KS}-{pro.lower()}-{epi.lower()}-nt{nt}-{co}", 1, TALL, 32 * KS, co, epi=epi,
                                         split=co // 2, pro=pro, modes=(mode,))
                by_nt = {}
                for co in range(COUT_STEP, COUT_MAX + 1, COUT_STEP):
                    f = form(lib, mk(co), mode)
                    if f is not None:
                        by_nt.setdefault(f["NT"], []).append(co)
                for nt, cos in sorted(by_nt.items()):
                    co = max(cos) if nt == 256 else min(cos)
                    out.append(mk(co, nt))
    return out


_TABLE = {}


def rows_cases(lib=None):
    """generated + edge + tile-walk cases (the generated ones need the library's host-side query; built once)"""
    if "all" not in _TABLE:
        if lib is None:
            from founddiff_amd import _lib as L
            lib = L.BF16.lib() if L.BF16.half_format == 0 else L.F16.lib()       # the plan does not depend on the 16-bit type
        _TABLE["gen"] = generated_cases(lib)
        _TABLE["all"] = _TABLE["gen"] + EDGE_CASES + WALK_CASES
    return _TABLE["all"]


# ------------------------------------------------------------------------------------------------ operands
SPECIAL_ROWS = ((0, 0, 0.0), (0, 5, 1.5), (-1, -1, -0.75), (0, 17, 0.0))        # (image, pixel, value of every channel)


def make_inputs(c, rq, seed=11):
    """conv_cases.make_inputs (sources, weight, bias, residual, gate, GroupNorm operands), plus the operands of the prologues and of
    the final form, on the CPU in fp32.  rq rounds what the library stores in its element type (also z and W_z)."""
    t = cc.make_inputs(conv_case(c), rq, seed)
    g = torch.Generator().manual_seed(seed + 1000)
    rn = lambda *s: torch.randn(*s, generator=g)
    K, P = c.cin, npx(c)
    if c.special:
        for b, m, v in SPECIAL_ROWS:
            t["in0"].view(c.B, P, c.ld0)[b, m] = v
            if c.pro == "ZRE":
                t["res"].view(c.B, P, c.ld_res)[b, m] = v
    if c.pro != "NONE":
        t["ln_gamma"], t["ln_beta"] = 1 + 0.3 * rn(K), 0.4 * rn(K)
        t["ln_mod"] = 0.5 * rn(c.B, c.ln_ld)
    if c.pro == "LN_GATE":
        t["z"] = rq(rn(c.B, P, c.ldz))
    if c.pro == "ZRE":
        CX = cx_of(c)
        t["zre_w"] = rq(rn(K, CX) / CX ** 0.5)
        t["zre_gamma"], t["zre_beta"] = 1 + 0.3 * rn(CX), 0.4 * rn(CX)
        t["zre_mod"] = 0.5 * rn(c.B, c.ln_ld)
    if c.epi == "GNSILU_ADD_FINAL":
        t["fin_w"] = rn(c.cout) / c.cout ** 0.5
        if c.fin_mode:
            t["fin_img"], t["fin_xin"] = rn(c.B, P).clamp(-1, 1), rn(c.B, P).clamp(-1, 1) * 0.5
    return t


def batch_slice(c, t, i):
    """(case, operands) of image i alone"""
    shared = {"bias", "gamma", "beta", "ln_gamma", "ln_beta", "zre_w", "zre_gamma", "zre_beta", "fin_w"}
    sl = {k: (v if k in shared else (v[:, i:i + 1] if k == "res" else (v[i:i + 1] if k != "weight" or c.wb else v))) for k, v in t.items()}
    return c._replace(B=1), sl


def column_slice(c, t, n):
    """(case, operands) of the first n output channels: the same leading weight rows, bias, gate and residual channels"""
    sl = dict(t, weight=t["weight"][:, :, :n].contiguous())
    if c.bias:
        sl["bias"] = t["bias"][:n].contiguous()
    return c._replace(cout=n, ldo=n), sl


# ------------------------------------------------------------------------------------------------ the reference
def _ln(x, eps):
    """LayerNorm over the last axis with the biased variance -> (normalised x, the same with every term replaced by its magnitude)"""
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    rstd = (var + eps).rsqrt()
    return (x - mean) * rstd, (x.abs() + mean.abs()) * rstd


def _mod(c, t, name, n, dt, dev, gamma, beta):
    """G = gamma (1 + scale), Bc = beta (1 + scale) + shift of adaLN rows [B, ld] holding shift | scale -> [B, 1, n] each, and the two
    with every term replaced by its magnitude: |gamma| (1 + |scale|), |beta| (1 + |scale|) + |shift|"""
    m = t[name].to(dev, dt)
    shift, scale = m[:, None, :n], m[:, None, n:2 * n]
    one = torch.ones(n, dtype=dt, device=dev)
    g = t[gamma].to(dev, dt) if c.affine else one
    b = t[beta].to(dev, dt) if c.affine else 0 * one
    return g * (1 + scale), b * (1 + scale) + shift, g.abs() * (1 + scale.abs()), b.abs() * (1 + scale.abs()) + shift.abs()


def _sources(c, t, dt, dev):
    P = npx(c)
    x = t["in0"].to(dev, dt).view(c.B, P, c.ld0)[..., c.off0:c.off0 + c.cin - c.c1]
    if c.c1:
        x = torch.cat((x, t["in1"].to(dev, dt).view(c.B, P, c.ld1)[..., c.off1:c.off1 + c.c1]), -1)
    return x


def prologue(c, t, dt, dev, z=None):
    """the fused prologue in the precision dt, as the kernels' comments define it -> dict: a [B, P, K] (the contraction's operand),
    abar (a with every term replaced by its magnitude; None without a prologue), and for ZRE ax / axbar (LNmod of the block input),
    lny (out_norm(y)).  z: ZRE's gate (default: computed here in dt from ax).
    abar = (|x| + |mean|) rstd Gbar + Bcbar, times |z| plus |local| for the gate forms.  Gbar and Bcbar are G = gamma (1 + scale) and
    Bc = beta (1 + scale) + shift term by term, not |G| and |Bc|: where beta (1 + scale) and shift cancel (or scale is near -1) the
    fp32 value of Bc (of G) is off by many of its own ulps, and a constant measured per unit of |Bc| would be that outlier's
    (1.8e-5 on this table, against 3.6e-7 per unit of the sum of magnitudes)."""
    x = _sources(c, t, dt, dev)
    if c.pro == "NONE":
        return dict(a=x, abar=None)
    n, nb = _ln(x, EPS)
    if c.pro == "LN_MOD":
        G, Bc, Gb, Bcb = _mod(c, t, "ln_mod", c.cin, dt, dev, "ln_gamma", "ln_beta")
        return dict(a=n * G + Bc, abar=nb * Gb + Bcb)
    g, be = t["ln_gamma"].to(dev, dt), t["ln_beta"].to(dev, dt)
    local = t["ln_mod"].to(dev, dt)[:, None, :c.cin]
    lny, lnyb = n * g + be, nb * g.abs() + be.abs()
    r = {}
    if c.pro == "LN_GATE":
        z = t["z"].to(dev, dt)[..., c.offz:c.offz + c.cin]
    else:
        xin = t["res"].to(dev, dt)[0][..., c.off_res:c.off_res + cx_of(c)]
        nx, nxb = _ln(xin, EPS)
        G, Bc, Gb, Bcb = _mod(c, t, "zre_mod", cx_of(c), dt, dev, "zre_gamma", "zre_beta")
        r.update(ax=nx * G + Bc, axbar=nxb * Gb + Bcb)
        if z is None:
            pre = r["ax"] @ t["zre_w"].to(dev, dt).T
            z = pre * torch.sigmoid(pre)
    r.update(a=lny * z + local, abar=lnyb * z.abs() + local.abs(), lny=lny, z=z)
    return r


# c_ln: the relative error of the prologue's own fp32 arithmetic per unit of abar.  MEASURED against the reference, never against the
# kernel: the largest |a32 - a64| / abar over every prologue case of this module (generated, edge, walk, batch, column), a32 the same
# formulas in fp32 torch (measure_c_ln below, on the CPU): 3.4e-7 on bfloat16 operands, 3.7e-7 on binary16, 2.03e-6 = 34 x 2^-24 on
# fp32 operands (zre128-one-row-noaffine-strided, image 1, pixel 4127, channel 21 of LNmod(x): an element with x and the row's mean
# both within 1e-3 of zero, where the mean's own rounding -- which scales with the row's typical |x| -- is all that is left; the
# 0.9999 quantile is 2.4e-7).  One constant for every mode: the largest.  The kernels sum in another order, in registers of four
# lanes, and the 16-bit z-recompute kernels take the variance in one pass: 4 x the measured value.
C_LN_MEASURED = 2.03e-6
C_LN_WORST = ("zre128-one-row-noaffine-strided", "fp32s")
C_LN = 4 * C_LN_MEASURED


def measure_c_ln(c, rq, dev="cpu"):
    """largest |a32 - a64| / abar of one case (ZRE: also of LNmod(block input); the gate z is the fp64 one in both evaluations, its own
    error is the dz term of the bound)"""
    t = make_inputs(c, rq)
    p64 = prologue(c, t, torch.float64, dev)
    p32 = prologue(c, t, torch.float32, dev, z=p64["z"].float() if c.pro == "ZRE" else None)
    worst = float(((p32["a"].double() - p64["a"]).abs() / p64["abar"]).max())
    if c.pro == "ZRE":
        worst = max(worst, float(((p32["ax"].double() - p64["ax"]).abs() / p64["axbar"]).max()))
    return worst


def c_mode(K, mode):
    """conv_cases.c_mode for a contraction over K channels"""
    return (K + 8) * 2.0 ** -24 + (2.0 ** -14 if mode == "fp32s" else 0.0)


def rows_reference(c, t, mode, tdt, dev):
    """The launch restated in fp64 on `dev` from the operands' stored values: the prologue, F.linear, bias and epilogue, the final dot
    and the sampler's update.  -> dict of fp64 tensors: out [B, P, Cout]; S = sum |w| |a| + |bias|; S_pro (the prologue's error carried
    through the contraction, see error_bounds); L, addend as conv_cases.conv_reference; for GNSILU_ADD_FINAL fin_out / fin_img [B, P]
    with fin_absdot = sum |fin_w ref|.  tdt: the stored element type (its unit roundoff is u_op and u_h)."""
    f64 = torch.float64
    D = lambda k: t[k].to(dev, f64)
    B, P, K, N = c.B, npx(c), c.cin, c.cout
    u_h = 0.0 if mode == "fp32s" else cc.U_OUT[tdt]       # rounding of a prologue result packed to 16 bits (fp32s: the split is in c_mode)
    pr = prologue(c, t, f64, dev)
    a = pr["a"]
    w = D("weight")[:, 0]                                   # [B or 1, Cout, K]
    lin = lambda x, m: torch.matmul(x, m.transpose(1, 2))   # broadcasts shared weights over the images
    v, S = lin(a, w), lin(a.abs(), w.abs())
    S_pro = torch.zeros_like(v)
    if c.pro != "NONE":
        E = u_h * a.abs() + C_LN * pr["abar"]
        if c.pro == "ZRE":
            # dz: the error of the recomputed gate, an absolute error of z.  u_h |z| is its rounding to the stored type (16-bit kernels;
            # the fp32s kernel keeps it in fp32 registers), the rest the z contraction's own error through SiLU (slope <= 1.1).
            # |LN(y)| dz enters the operand's error as it is: c_ln scales the prologue's own arithmetic, not an operand's error.
            wz = D("zre_w")
            Sz = pr["ax"].abs() @ wz.abs().T
            Sz_pro = (u_h * pr["ax"].abs() + C_LN * pr["axbar"]) @ wz.abs().T
            dz = u_h * pr["z"].abs() + 1.1 * (c_mode(cx_of(c), mode) * Sz + Sz_pro)
            E = E + pr["lny"].abs() * dz
        S_pro = lin(E, w.abs())
    if c.bias:
        v, S = v + D("bias"), S + D("bias").abs()
    L, addend = torch.ones(1, 1, N, dtype=f64, device=dev), torch.zeros_like(v)
    silu = lambda z: z * torch.sigmoid(z)
    if c.epi == "RELU":
        out = v.clamp(min=0)
    elif c.epi == "SILU_SPLIT":
        out = torch.cat((v[..., :c.split], silu(v[..., c.split:])), -1)
        L = torch.where(torch.arange(N, device=dev) >= c.split, 1.1, 1.0).to(f64).view(1, 1, -1)
    elif c.epi in ("GATE_RES", "RES_RELU"):
        addend = D("res")[0][..., c.off_res:c.off_res + N]
        if c.epi == "GATE_RES":
            gate = D("gate")[:, None, :N]
            out, L = addend + gate * v, gate.abs()
        else:
            out = (v + addend).clamp(min=0)
    elif c.epi in ("GNSILU_ADD", "GNSILU_ADD_FINAL"):
        mr = D("gn").repeat_interleave(N // c.groups, 1)                  # [B, Cout, 2]
        addend = silu((D("h") - mr[:, None, :, 0]) * mr[:, None, :, 1] * D("gamma") + D("beta"))
        out = v + addend
    else:
        out = v
    r = dict(out=out, S=S, S_pro=S_pro, L=L, addend=addend.abs())
    if c.epi == "GNSILU_ADD_FINAL":
        fw = D("fin_w")
        o = out @ fw + FIN_B
        r.update(fin_out=o, fin_absdot=out.abs() @ fw.abs())
        if c.fin_mode:
            prd = o.clamp(-1, 1)
            r["fin_img"] = (D("fin_xin") - prd).clamp(-1, 1) if c.fin_last else D("fin_img") - FIN_ALPHA * prd
    return r


def error_bounds(c, mode, ref, out_dtype):
    """bound of a stored element, from the inputs alone:
        u_out |ref| + L (c_mode S + S_pro) + 2^-20 (|ref| + |addend|)
    conv_cases.error_bounds with the prologue's term: S_pro = sum_k |w_nk| (u_op |a_k| + c_ln abar_k [+ |LN(y)_k| dz_k for ZRE])."""
    pre = ref["L"] * (c_mode(c.cin, mode) * ref["S"] + ref["S_pro"]) + 2.0 ** -20 * (ref["out"].abs() + ref["addend"])
    return cc.U_OUT[out_dtype] * ref["out"].abs() + pre


def final_bounds(c, t, ref, bound, dev):
    """(bound of fin_out, bound of fin_img or None): sum_n |fin_w_n| bound_n -- the store rounding of each block output included, it is
    the kernel's rounding point -- + (Cout + 4) 2^-24 sum |fin_w_n ref_n|.  Clamping is 1-Lipschitz; the update adds |fin_alpha| times
    that (1 times in the last step), + 2^-23 (|fin_img| + |x_in| + 1) for the two fp32 operations of the update itself."""
    fw = t["fin_w"].to(dev, torch.float64).abs()
    bo = bound @ fw + (c.cout + 4) * 2.0 ** -24 * ref["fin_absdot"]
    if not c.fin_mode:
        return bo, None
    arith = 2.0 ** -23 * (t["fin_img"].to(dev, torch.float64).abs() + t["fin_xin"].to(dev, torch.float64).abs() + 1)
    return bo, (1.0 if c.fin_last else FIN_ALPHA) * bo + arith
