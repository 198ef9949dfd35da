"""fd_conv_form (host only): which implicit-GEMM tile, and which loader, fd_conv2d launches.  No GPU.

tests/conv_cases.CONV_CASES, the shapes tests/test_gpu_conv_forms.py runs, reach every one of the 28 instantiations of conv_igemm_kernel
(tile ids 0 .. 6 x bf16 pointwise loader / bf16 general gather / fp32 / split fp32) and every tiling edge, operand layout and epilogue
path of the coverage list below -- asserted from the query's answers and the case fields, so a dropped case or a moved dispatch
threshold names what lost its test."""
import ctypes as C
import os

import pytest
import torch

import conv_cases as cc
from conv_cases import BATCH_CASES, CONV_CASES, PW_GENERAL_CASES, case_id, expected_form, form, tile_geom


@pytest.fixture(scope="module")
def lib():
    for var in ("FD_CONV_KID", "FD_CONV_BIG_TILE"):
        assert var not in os.environ, (f"{var} is set: a development build of the library would force a tile and this module (and "
                                       "tests/test_gpu_conv_forms.py) would test another dispatch than the shipped one -- unset it")
    from founddiff_amd import _lib as L
    return L.lib()


def _rows(lib):
    """(case, mode, tile geometry) of every run of the GPU test"""
    return [(c, m, tile_geom(c, m, form(lib, c, m))) for c in CONV_CASES for m in c.modes]


# the cases the table was specified with: most items of the coverage list are reached by more than one of them, so the coverage test
# alone would let one go
MINIMUM_CASES = """tall-pw-96 tall-3x3-96-relu-stats tall-e-3x3-72-stats tall-pw-64-gate-f32 tall-e-40-silu20-stats tall-pw-24-gnsilu
tall-pw-32-resrelu-slices tall-xproj-12 tall-4x4s2-16-stats id4-pw-512-silu id5-pw-512-resrelu id4-3x3-264 id5-3x3-264-gate pw-136-silu64
pw-128-gnsilu up-3x3-72-resrelu 3x3-200-stats pw-40-relu pw-64-f32-slices pw-64-gate pw-64-resrelu 7x7-4-stats cat-3x3-64-gate-stats
4x4s2-128 wbatch-32-gate xproj-tiny-12 3x3-24-none 3x3-24-silu_split 3x3-24-relu 3x3-24-gate_res 3x3-24-res_relu 3x3-24-gnsilu_add
3x3-20-none 3x3-20-silu_split 3x3-20-relu 3x3-20-gate_res 3x3-20-res_relu 3x3-20-gnsilu_add""".split()


def test_case_table_is_well_formed(lib):
    ids = [case_id(c) for c in CONV_CASES]
    assert len(ids) == len(set(ids)), "duplicate case"
    assert set(MINIMUM_CASES) <= set(ids), sorted(set(MINIMUM_CASES) - set(ids))
    for c in CONV_CASES:
        assert set(c.modes) == set(cc.ALL), case_id(c)
        assert c.B <= 2, case_id(c)
        el = 8                                  # what fd_conv2d requires of every mode the case runs in (16-bit: multiples of 8)
        assert (c.cin - c.c1) % el == 0 and c.c1 % el == 0 and c.ld0 % el == 0 and c.off0 % el == 0 and c.ld1 % el == 0 and c.off1 % el == 0
        assert c.off0 + c.cin - c.c1 <= c.ld0 and c.off1 + c.c1 <= c.ld1 and c.offo + c.cout <= c.ldo, case_id(c)
        assert c.off_res + c.cout <= c.ld_res and c.cout <= c.gate_ld
        assert not (c.stats and c.ndir > 1)     # the sums are indexed by image, not by direction
        if c.epi == "GNSILU_ADD":
            assert c.groups > 0 and c.cout % c.groups == 0


def test_every_case_runs_the_form_it_expects(lib):
    """... and no case is taken by another kernel: not the streaming row-GEMM (fd_conv_prologue_ok), not the 3x3 family (11 .. 16), not
    the persistent pointwise GEMM (7)"""
    twins = [(c._replace(B=1, expect=dict(c.expect, kid=kid1)), m) for c, kid1 in BATCH_CASES for m in cc.BATCH_MODES]
    pwg = [(x, "bf16") for c in PW_GENERAL_CASES for x in (c, cc.split_sources(c, {"in0": None})[0])]
    for c, m in [(c, m) for c in CONV_CASES for m in c.modes] + [(c, m) for c, _ in BATCH_CASES for m in cc.BATCH_MODES] + twins + pwg:
        p = cc.params_for(c, m, cc.DUMMY_PTRS)
        assert lib.fd_conv_prologue_ok(C.byref(p)) == 0, (case_id(c), m, "runs on the streaming row-GEMM")
        kid = lib.fd_conv_kernel_id(C.byref(p))
        assert 0 <= kid <= 6, (case_id(c), m, f"runs on kernel {kid}, not on the implicit GEMM")
        got = lib.fd_conv_form(C.byref(p))
        assert got & 0xFF == kid and got >> 8 in (0, 1)
        assert got == expected_form(c, m), (case_id(c), m, f"form {got:#x}, the table says {expected_form(c, m):#x}")
        if m != "bf16":
            assert got >> 8 == 0, "the pointwise loader is a 16-bit form"


def test_engine_probe_form(lib):
    """DAEngine.conv(probe="form") poses the same question"""
    from founddiff_amd import _lib as L
    from founddiff_amd.engine import _T, DAEngine

    class Bare(DAEngine):
        def __init__(self, mode):
            self.mode, self.hip, self.dev, self.buf = mode, L.BF16, torch.device("cpu"), {}
            self.dt, self.tdt = _T[mode]
            self.f32_split = int(mode == "fp32s")
    for name in ("pw-40-relu", "tall-pw-96", "tall-3x3-96-relu-stats", "4x4s2-128", "id5-pw-512-resrelu"):
        c = next(x for x in CONV_CASES if x.name == name)
        for m in c.modes:
            e = Bare(m)
            z = torch.zeros(16, dtype=e.tdt)
            zf = torch.zeros(16)
            kw = dict(c0=c.cin - c.c1, ld0=c.ld0, off0=c.off0, in1=z if c.c1 else None, c1=c.c1, ld1=c.ld1, off1=c.off1, stride=c.stride,
                      pad=c.pad, weight=z, bias=zf if c.bias else None, Cout=c.cout, KH=c.k, KW=c.k, epi=cc.EPIS.index(c.epi),
                      res=z if c.epi in ("GATE_RES", "RES_RELU") else None, stats=zf if c.stats else None, ldo=c.ldo, offo=c.offo,
                      out_f32=c.out_f32, split=c.split, ld_res=c.ld_res, off_res=c.off_res)
            assert e.conv(None, z, c.B, c.H, c.W, z, probe="form", **kw) == form(lib, c, m) == expected_form(c, m), (name, m)
            assert e.conv(None, z, c.B, c.H, c.W, z, probe="kid", **kw) == c.expect["kid"]


def features(c, m, g):
    """the items of the coverage list that (case, mode) reaches on the tile `g` the dispatcher chose"""
    f = set()
    P, K, BM, BN, BK = cc.ohw(c), g["K"], g["BM"], g["BN"], g["BK"]
    kind = ("bf16-pw" if g["pw"] else "bf16-general") if m == "bf16" else m
    f.add(f"tile {g['kid']} {kind}")
    if g["kid"] == 6 and g["pw"]:
        assert not g["pwe"]
        f.add("tile 6 PW loader + staged epilogue")
    # M edges
    if P % BM:
        f.add("M: OH.OW not a multiple of BM")
    empty_band = BM >= 128 and 0 < P % BM <= BM - 64                  # the last tile has a 64-row band with no pixel in it
    if empty_band:
        f.add("M: last tile's second band empty")
    if P < BM:
        f.add("M: OH.OW < BM")
    # N edges
    if c.cout % BN:
        f.add("N: Cout not a multiple of BN")
    if c.cout % 8:
        f.add("N: Cout not a multiple of 8")
        if c.cout == 12 and c.ndir == 4:
            f.add("N: Cout 12 x_proj")
    if c.cout < 8:
        f.add("N: Cout < 8")
    # K edges (the general loader's; the pointwise loader needs whole tiles)
    if not g["pw"]:
        if K % BK:
            f.add("K: not a multiple of BK")
        if c.cin < BK and c.k > 1:
            f.add("K: Cin < BK, a tile spans several taps")
        if c.cin > BK and c.cin % BK and c.k > 1:
            f.add("K: Cin not a multiple of BK, tiles straddle a tap")
        if cc.k_paths(c, BK) == {"counter", "decode"}:
            f.add("K: general decode and counter path in one launch")
    # sources
    if c.c1:
        c0 = c.cin - c.c1
        if g["pw"]:
            assert c0 % BK == 0
            f.add("src: c0 on a K-tile boundary (PW)")
        elif c0 % BK:
            f.add("src: c0 inside a K tile (general)")
    if c.ld0 > c.cin - c.c1 and c.off0 > 0:
        f.add("src: ld0 > c0, off0 > 0")
    if c.c1 and c.ld1 > c.c1 and c.off1 > 0:
        f.add("src: ld1 > c1, off1 > 0")
    if c.wb and c.B == 2:
        f.add("src: per-image weights")
    # geometry
    if c.ndir == 1 and not c.up:
        f.add(f"geo: k{c.k} s{c.stride} p{c.pad}")
    if c.up:
        f.add("geo: nearest x2 up-sampling")
    if c.ndir == 4:
        assert c.stride == 2
        f.add("geo: ndir 4 tall, odd source" if BM == 128 and (c.H | c.W) & 1 else "geo: ndir 4 tiny" if P < 64 else "geo: ndir 4")
    # output
    if c.ldo > c.cout and c.offo > 0:
        f.add("out: ldo > Cout, offo > 0")
    if c.out_f32 and m == "bf16":
        f.add("out: fp32 from 16 bits, " + ("PWE" if g["pwe"] else "staged"))
    # epilogues
    path = "PWE" if g["pwe"] else ("staged-vector" if cc.vec_ok(c) else "staged-scalar")
    f.add(f"epi: {c.epi} {path}")
    if c.epi == "SILU_SPLIT":
        f.add(f"epi: SILU_SPLIT split % 8 {'==' if c.split % 8 == 0 else '!='} 0, {'PW' if g['pw'] else 'general'}")
    if c.epi == "GATE_RES" and c.gate_ld > c.cout:
        f.add("epi: gate_ld > Cout")
    if c.epi in ("GATE_RES", "RES_RELU") and c.ld_res > c.cout and c.off_res > 0:
        f.add("epi: ld_res > Cout, off_res > 0")
    # GroupNorm partial sums
    if c.stats:
        assert not g["pw"] and g["kid"] not in (4, 5)
        f.add(f"stats: tile {g['kid']}")
        f.add("stats: BM 64, two passes per band" if g["TMW"] == 32 else "stats: BM 128")
        if P % 64:
            f.add("stats: ragged last band")
        if empty_band:
            f.add("stats: empty last band")
        if c.cout % BN:
            f.add("stats: ragged Cout")
        if c.epi != "NONE":
            f.add("stats: after a non-trivial epilogue")
    return f


H16, ANY = ("bf16",), cc.ALL
# (item, the element modes that must each reach it)
REQUIRED = (
    [(f"tile {k} {kind}", (m,)) for k in range(7) for kind, m in (("bf16-pw", "bf16"), ("bf16-general", "bf16"), ("fp32", "fp32"),
                                                                  ("fp32s", "fp32s"))]
    + [("tile 6 PW loader + staged epilogue", H16)]
    + [(x, ANY) for x in ("M: OH.OW not a multiple of BM", "M: last tile's second band empty", "M: OH.OW < BM",
                          "N: Cout not a multiple of BN", "N: Cout not a multiple of 8", "N: Cout 12 x_proj", "N: Cout < 8",
                          "K: not a multiple of BK", "K: Cin < BK, a tile spans several taps",
                          "K: Cin not a multiple of BK, tiles straddle a tap", "K: general decode and counter path in one launch",
                          "src: c0 inside a K tile (general)", "src: ld0 > c0, off0 > 0", "src: ld1 > c1, off1 > 0",
                          "src: per-image weights",
                          "geo: k1 s1 p0", "geo: k3 s1 p1", "geo: k4 s2 p1", "geo: k7 s1 p3", "geo: nearest x2 up-sampling",
                          "geo: ndir 4 tall, odd source", "geo: ndir 4 tiny", "out: ldo > Cout, offo > 0")]
    + [("src: c0 on a K-tile boundary (PW)", H16), ("out: fp32 from 16 bits, PWE", H16), ("out: fp32 from 16 bits, staged", H16)]
    + [(f"epi: {e} PWE", H16) for e in cc.EPIS]
    + [(f"epi: {e} {p}", ANY) for e in cc.EPIS for p in ("staged-vector", "staged-scalar")]
    + [("epi: SILU_SPLIT split % 8 != 0, general", ANY), ("epi: SILU_SPLIT split % 8 == 0, PW", H16), ("epi: gate_ld > Cout", ANY),
       ("epi: ld_res > Cout, off_res > 0", ANY)]
    + [(x, ANY) for x in ("stats: BM 64, two passes per band", "stats: tile 0", "stats: tile 1", "stats: tile 6",
                          "stats: ragged last band", "stats: empty last band", "stats: ragged Cout",
                          "stats: after a non-trivial epilogue")]
)


def test_cases_reach_every_form(lib):
    reached = {}
    for c, m, g in _rows(lib):
        for item in features(c, m, g):
            reached.setdefault(item, {}).setdefault(m, []).append(case_id(c))
    lost = [f"{item} [{m}]" for item, modes in REQUIRED for m in modes if not reached.get(item, {}).get(m)]
    assert not lost, "no case of tests/conv_cases.CONV_CASES reaches: " + "; ".join(lost)
    # the 128-row sums on ids 0 and 1 and the id-6 sums at Cout <= 32, each with both kinds of last band somewhere
    for k in (0, 1, 6):
        assert set(reached[f"stats: tile {k}"]) == set(cc.ALL)
    assert any(c.cout <= 32 for c in CONV_CASES if c.stats and c.expect["kid"] == 6)
