"""fd_pw_dw3x3_plan (host only): which of the eight fused LN -> 1x1 -> depthwise 3x3 kernels a launch runs, how many consecutive tiles a
workgroup walks and on which grid -- and the CPU check of tests/pwdw_cases.error_bounds.  No GPU.

tests/pwdw_cases.CASES, the shapes tests/test_gpu_pwdw_forms.py runs, reach all eight kernels, every tiles-per-workgroup value of every
entry point once with an exact and once with a ragged last workgroup, and the first and last depthwise chunk count and weight-group
count of each Cin -- asserted from the query's answers.  What must be reached is written out as literals here, so a dropped case or a
moved threshold names what lost its test.  The plan refuses exactly where the _ok queries do, and every _nblk query is its grid x.

The bound is checked before any kernel is asked: pwdw_cases.restate (fp32 torch with the kernels' rounding points) stays inside it on
every case and on both 16-bit types, and leaves it with each of three seeded faults."""
import itertools
import os

import pytest
import torch

import pwdw_cases as pc
from pwdw_cases import CASES, DW, DWGRAM, F32, GRAM, GRAM32, PROJ, PROJ32, case_id

BF16, F32T, LL = pc.FD_BF16, pc.FD_F32, pc.LOW_LATENCY


@pytest.fixture(scope="module")
def lib():
    for var in ("FD_PWDW_TPW", "FD_GRAM_TPW", "FD_PWDW_MINPIX", "FD_NO_PWDW128", "FD_NO_PWDW_PROJ", "FD_NO_GRAM_FUSE", "FD_NO_DWGRAM"):
        assert var not in os.environ, (f"{var} is set: a development build of the library would plan other launches than the shipped "
                                       "one -- unset it")
    from founddiff_amd import _lib as L
    return L.lib()


KERNELS = ("pwdw_kernel<64>", "pwdw_kernel<128>", "pwdw_kernel<64, PROJ>", "pwdw_gram_kernel", "dwconv_gram_kernel",
           "pwdw32_kernel<DW, 16>", "pwdw32_kernel<GRAM, 8>", "pwdw32_kernel<PROJ, 8>")
# entry point -> the tiles per workgroup its launches can take in the shipped build
TPW = {DW: (1, 4), PROJ: (1, 4), GRAM: (8, 4), DWGRAM: (1, 2, 4), F32: (1, 4), GRAM32: (16,), PROJ32: (2, 8)}
# kernel -> (fewest, most) depthwise chunks and 32-row weight groups per tile among the forms the table was specified with
CHUNKS = {"pwdw_kernel<64>": (1, 3), "pwdw_kernel<128>": (1, 4), "pwdw32_kernel<DW, 16>": (1, 4)}
WGROUPS = {"pwdw_kernel<64>": (2, 8), "pwdw_kernel<128>": (3, 16), "pwdw32_kernel<DW, 16>": (1, 4)}
# (Cin, Cdw, Cz, SiLU) of fd_pw_dw3x3 that must be launched
DW_FORMS = [(64, 128, 128, True), (64, 128, 0, True), (64, 192, 0, False), (64, 64, 0, True), (64, 64, 32, False), (64, 128, 96, True),
            (128, 256, 256, True), (128, 256, 0, True), (128, 64, 32, False), (128, 192, 64, False)]
# the cases the table was specified with: most items of the coverage lists are reached by more than one of them, so the coverage tests
# alone would let one go
MINIMUM_CASES = """dw64-128-128-b4-r3 dw64-128-0-silu-b1 dw64-192-0-b4-exact dw64-64-0-b1-row dw64-64-32-b4-r1 dw64-128-96-b1-col dw64-strided
dw64-special dw64-range-hi dw64-range-lo dw128-256-256-b4-r3 dw128-256-0-b1 dw128-64-32-b4-exact dw128-192-64-b1-r1 dw128-strided
dw128-special dw128-range-hi dw128-range-lo proj-b1-exact proj-b4-r3 proj-b4-row-affine proj-strided proj-special proj-range-hi
proj-range-lo gram-v-exact gram-nov-r3 gram-v-row-affine gram-nov-col gram-ll-v-r1 gram-ll-nov-exact gram-strided gram-special
gram-range-hi gram-range-lo dwgram-1tile-c64 dwgram-64t-c128 dwgram-63t-c64 dwgram-63t-c320 dwgram-256t-c128 dwgram-255t-c64
dwgram-323t-c64 dwgram-special dwgram-range-hi dwgram-range-lo f32-32-b1 f32-64-b4-r2 f32-96-b1-row f32-128-b4-exact f32-128-b1-col
f32-strided f32-special gram32-exact gram32-r3 gram32-row-affine gram32-col gram32-strided gram32-special proj32-b1-exact proj32-b1-r3
proj32-b4-r3 proj32-b4-exact-affine proj32-b1-col proj32-b2-row proj32-strided proj32-special gram-sparse dwgram-sparse
gram32-sparse""".split()


def _plans(lib, cases=CASES):
    return [(c, pc.plan(lib, c)) for c in cases]


def test_case_table_is_well_formed(lib):
    ids = [case_id(c) for c in CASES]
    assert len(ids) == len(set(ids)), "duplicate case"
    assert set(MINIMUM_CASES) <= set(ids), "dropped: " + " ".join(sorted(set(MINIMUM_CASES) - set(ids)))
    assert set(pc.REPEAT) <= set(ids)
    for c, pl in _plans(lib, CASES + pc.BATCH_CASES + pc.CROSS_CASES):
        n, ge = case_id(c), pc.geom(c)
        assert pl is not None, f"{n}: refused by {c.entry}'s _ok query"
        assert c.B <= 4 and pc.npx(c) <= 41344, n
        assert pl["ntiles"] == (c.H // 8) * (c.W // pl["TW"]) and pl["gx"] == -(-pl["ntiles"] // pl["tpw"]), (n, pl)
        assert (pl["gy"], pl["gz"]) == ((c.C // 64, c.B) if c.entry == DWGRAM else (c.B, 1)), (n, pl)
        for v in (ge.ld_x, ge.off_x, ge.ld_dw, ge.off_dw, ge.ld_z, ge.off_z, ge.ld_qkv):
            assert v % ge.unit == 0, (n, v)
        assert ge.gate_ld % 4 == 0 and ge.ld_wdw % 4 == 0, n
        if c.strided:
            assert ge.off_x and ge.off_dw and (ge.off_z or not c.cz) and ge.ln_ld > 2 * c.cin and ge.gate_ld > 64, n
            assert (ge.shift_off, ge.scale_off, ge.gate_off) == (3 * c.cin, 4 * c.cin, 5 * c.cin), n
        if c.entry == DWGRAM:
            assert ge.ld_qkv > 3 * c.C, n


def test_cases_reach_every_kernel(lib):
    reached = {}
    for c, pl in _plans(lib):
        reached.setdefault(pl["kernel"], []).append(case_id(c))
    missing = [k for k in KERNELS if k not in reached]
    assert not missing, f"no case launches {missing}"
    assert set(reached) <= set(KERNELS), set(reached) - set(KERNELS)
    # ... and the entry points run the kernels their names say
    expect = {PROJ: KERNELS[2], GRAM: KERNELS[3], DWGRAM: KERNELS[4], F32: KERNELS[5], GRAM32: KERNELS[6], PROJ32: KERNELS[7]}
    for c, pl in _plans(lib):
        assert pl["kernel"] == expect.get(c.entry, KERNELS[0] if c.cin == 64 else KERNELS[1]), (case_id(c), pl)


def test_every_tile_walk_exact_and_ragged(lib):
    """each tiles-per-workgroup value of each entry point: once with a full last workgroup and (above one tile) once with a ragged one"""
    reached = {}
    for c, pl in _plans(lib):
        assert pl["tpw"] in TPW[c.entry], f"{case_id(c)}: {c.entry} walks {pl['tpw']} tiles per workgroup -- not in this file's list"
        reached.setdefault((c.entry, pl["tpw"], "exact" if pl["ntiles"] % pl["tpw"] == 0 else "ragged"), []).append(case_id(c))
    want = [(e, tpw, kind) for e, tpws in TPW.items() for tpw in tpws for kind in ("exact", "ragged") if tpw > 1 or kind == "exact"]
    missing = [w for w in want if w not in reached]
    assert not missing, f"no case for (entry point, tiles per workgroup, last workgroup): {missing}"
    # a ragged last workgroup of every size the shapes were chosen for: 3 tiles and 1 tile left
    left = {(c.entry, pl["tpw"]): set() for c, pl in _plans(lib)}
    for c, pl in _plans(lib):
        left[(c.entry, pl["tpw"])].add(pl["ntiles"] % pl["tpw"])
    for key, n in (((DW, 4), 3), ((DW, 4), 1), ((PROJ, 4), 3), ((PROJ, 4), 1), ((GRAM, 8), 3), ((GRAM, 8), 1), ((GRAM, 4), 1), ((F32, 4), 2),
                   ((GRAM32, 16), 3), ((PROJ32, 8), 3), ((PROJ32, 2), 1)):
        assert n in left[key], f"{key}: no case whose last workgroup holds {n} tiles (have {sorted(left[key])})"
    # fd_dwconv_gram's thresholds: 63 and 64 tiles, 255 and 256
    nt = {(pl["ntiles"], pl["tpw"]) for c, pl in _plans(lib) if c.entry == DWGRAM}
    assert {(1, 1), (63, 1), (64, 2), (255, 2), (256, 4), (323, 4)} <= nt, nt
    assert {c.C for c in CASES if c.entry == DWGRAM} >= {64, 128, 320}


def test_first_and_last_chunk_and_group_counts(lib):
    got_c, got_w = {}, {}
    for c, pl in _plans(lib):
        got_c.setdefault(pl["kernel"], set()).add(pl["chunks"])
        got_w.setdefault(pl["kernel"], set()).add(pl["wgroups"])
        if c.entry == DW:
            assert (pl["chunks"], pl["wgroups"]) == (c.cdw // 64, (c.cdw + c.cz) // 32), (case_id(c), pl)
        if c.entry == F32:
            assert pl["chunks"] == pl["wgroups"] == c.cdw // 32, (case_id(c), pl)
    for k, (lo, hi) in CHUNKS.items():
        assert {lo, hi} <= got_c[k], f"{k}: depthwise chunk counts {sorted(got_c[k])}, wanted {lo} and {hi}"
    for k, (lo, hi) in WGROUPS.items():
        assert {lo, hi} <= got_w[k], f"{k}: weight-group counts {sorted(got_w[k])}, wanted {lo} and {hi}"
    assert got_c[KERNELS[5]] >= {1, 2, 3, 4}, "fd_pw_dw3x3_f32 at Cdw 32, 64, 96 and 128"


def test_forms_and_switches(lib):
    have = {(c.cin, c.cdw, c.cz, c.silu) for c in CASES if c.entry == DW}
    have_any = {(c.cin, c.cdw, c.cz) for c in CASES if c.entry == DW}
    for f in DW_FORMS:
        assert f in have or (f[:3] in have_any and not f[3]), f"fd_pw_dw3x3 form (Cin, Cdw, Cz, SiLU) {f} has no case"
    assert (64, 128, 0, True) in have, "Cz = 0 with SiLU: the z-recompute route"
    for e in (DW, F32):
        for field in ("affine", "bias", "silu"):
            assert {getattr(c, field) for c in CASES if c.entry == e} == {True, False}, f"{e}: {field} in one state only"
    for e in pc.ENTRIES:
        mine = [c for c in CASES if c.entry == e]
        assert any(c.special for c in mine), f"{e}: no special case"
        assert e not in (GRAM, DWGRAM, GRAM32) or any(c.sparse for c in mine), f"{e}: no sparse case"
        if e != DWGRAM:
            assert any(c.strided for c in mine), f"{e}: no strided case"
        if not pc.is32(mine[0]):
            assert {c.rng for c in mine} >= {"hi", "lo"}, f"{e}: no range case"
    for k in KERNELS[:2]:
        mine = [c for c, pl in _plans(lib) if pl["kernel"] == k]
        assert any(c.special for c in mine) and any(c.strided for c in mine) and {c.rng for c in mine} >= {"hi", "lo"}, k
    for e in (DW, PROJ, F32, PROJ32):
        assert {c.B for c in CASES if c.entry == e} >= {1, 4}, f"{e}: B = 1 and B = 4"
    assert {(c.out_v, c.lowlat) for c in CASES if c.entry == GRAM} == set(itertools.product((True, False), repeat=2))
    assert {case_id(c) for c in pc.BATCH_CASES} >= {"inv-dw64", "inv-dw128", "inv-proj", "inv-gram", "inv-dwgram", "inv-f32", "inv-gram32",
                                                    "inv-proj32"} and all(c.B == 4 for c in pc.BATCH_CASES)


SHAPES = [(128, 256), (8, 4096), (2048, 16), (120, 256), (128, 248), (132, 256), (256, 136), (264, 144), (128, 128), (120, 128), (128, 120),
          (136, 152), (132, 128), (8, 2048), (2048, 8), (1024, 16), (64, 128), (8, 16), (72, 112), (16, 8), (12, 16), (4096, 4096)]


def _ok(lib, entry, opts, cin, cdw, cz, C_, H, W):
    return {DW: lambda: lib.fd_pw_dw3x3_ok(opts, cin, cdw, cz, H, W), PROJ: lambda: lib.fd_pw_dw3x3_proj_ok(opts, cin, H, W),
            GRAM: lambda: lib.fd_pw_dw3x3_gram_ok(opts, cin, H, W), DWGRAM: lambda: lib.fd_dwconv_gram_ok(opts, C_, H, W),
            F32: lambda: lib.fd_pw_dw3x3_f32_ok(opts, cin, cdw, H, W), GRAM32: lambda: lib.fd_pw_dw3x3_gram_f32_ok(opts, cin, H, W),
            PROJ32: lambda: lib.fd_pw_dw3x3_proj_f32_ok(opts, cin, H, W)}[entry]()


def test_plan_refuses_exactly_where_the_ok_queries_do(lib):
    from founddiff_amd import _lib as L
    n = 0
    for entry in pc.ENTRIES:
        cdws = (0, 32, 48, 64, 96, 128, 160, 192, 256, 320) if entry in (DW, F32) else (0,)
        czs = (0, 16, 32, 96, 256, 288, -32) if entry == DW else (0,)
        Cs = (0, 32, 64, 96, 128, 320) if entry == DWGRAM else (0,)
        cins = (64,) if entry == DWGRAM else (32, 64, 96, 128, 256)
        for opts, cin, cdw, cz, C_, (H, W), B in itertools.product((BF16, F32T, BF16 | LL, F32T | LL), cins, cdws, czs, Cs, SHAPES, (1, 4)):
            # (the fixed-width entries: the widths their _ok queries assume)
            a = dict(Cdw={PROJ: 64, GRAM: 192}.get(entry, cdw), Cz=cz)
            pl = L.pwdw_plan(lib, entry, opts, cin, a["Cdw"], a["Cz"], C_, B, H, W)
            ok = bool(_ok(lib, entry, opts, cin, cdw, cz, C_, H, W))
            assert (pl is not None) == ok, f"{entry} opts={opts:#x} Cin={cin} Cdw={cdw} Cz={cz} C={C_} B={B} {H}x{W}: plan {pl}, _ok {ok}"
            n += 1
    assert n > 10000


# (entry, dtype_opts, Cin, Cdw, Cz, C, (H, W)) -> served; the thresholds, one line each
THRESHOLDS = [
    ((DW, BF16, 64, 192, 0, 0, (128, 256)), True), ((DW, BF16, 64, 256, 0, 0, (128, 256)), False),      # Cdw <= 192 at Cin 64
    ((DW, BF16, 128, 256, 256, 0, (128, 256)), True), ((DW, BF16, 128, 320, 0, 0, (128, 256)), False),  # Cdw, Cz <= 256 at Cin 128
    ((DW, BF16, 128, 256, 288, 0, (128, 256)), False),
    ((DW, BF16, 64, 96, 0, 0, (128, 256)), False), ((DW, BF16, 64, 64, 16, 0, (128, 256)), False),      # Cdw % 64, Cz % 32
    ((DW, BF16, 64, 64, 608, 0, (128, 256)), True),                                                       # (no Cz limit at Cin 64)
    ((DW, BF16 | LL, 128, 256, 256, 0, (128, 256)), False), ((DW, BF16 | LL, 64, 128, 128, 0, (128, 256)), True),   # C = 128 under low latency
    ((DW, BF16, 64, 128, 0, 0, (120, 256)), False), ((DW, BF16, 64, 128, 0, 0, (8, 4096)), True),        # 32768 px
    ((DW, BF16, 64, 128, 0, 0, (256, 136)), False), ((DW, BF16, 64, 128, 0, 0, (132, 256)), False),      # W % 16, H % 8
    ((DW, F32T, 64, 128, 0, 0, (128, 256)), False),
    ((PROJ, BF16, 64, 0, 0, 0, (128, 256)), True), ((PROJ, BF16 | LL, 64, 0, 0, 0, (128, 256)), False), ((PROJ, BF16, 128, 0, 0, 0, (128, 256)), False),
    ((PROJ, BF16, 64, 0, 0, 0, (120, 256)), False),
    ((GRAM, BF16, 64, 0, 0, 0, (128, 256)), True), ((GRAM, BF16 | LL, 64, 0, 0, 0, (128, 256)), True), ((GRAM, BF16, 128, 0, 0, 0, (128, 256)), False),
    ((GRAM, BF16, 64, 0, 0, 0, (120, 256)), False),
    ((DWGRAM, BF16, 0, 0, 0, 64, (8, 16)), True), ((DWGRAM, BF16, 0, 0, 0, 96, (8, 16)), False), ((DWGRAM, BF16, 0, 0, 0, 320, (72, 112)), True),
    ((DWGRAM, BF16, 0, 0, 0, 64, (12, 16)), False), ((DWGRAM, BF16, 0, 0, 0, 64, (16, 8)), False), ((DWGRAM, BF16, 0, 0, 0, 64, (4096, 4096)), False),
    ((F32, F32T, 64, 32, 0, 0, (128, 128)), True), ((F32, F32T, 64, 128, 0, 0, (128, 128)), True), ((F32, F32T, 64, 160, 0, 0, (128, 128)), False),
    ((F32, F32T, 64, 48, 0, 0, (128, 128)), False), ((F32, F32T, 64, 64, 0, 0, (120, 128)), False),                     # 16384 px
    ((F32, F32T, 64, 64, 0, 0, (136, 152)), False), ((F32, BF16, 64, 64, 0, 0, (128, 128)), False), ((F32, F32T, 128, 64, 0, 0, (128, 128)), False),
    ((GRAM32, F32T, 64, 0, 0, 0, (136, 152)), True), ((GRAM32, F32T, 64, 0, 0, 0, (120, 128)), False), ((GRAM32, F32T, 64, 0, 0, 0, (2048, 8)), True),
    ((GRAM32, F32T, 64, 0, 0, 0, (132, 128)), False),
    ((PROJ32, F32T, 64, 0, 0, 0, (136, 152)), True), ((PROJ32, F32T, 64, 0, 0, 0, (120, 128)), False), ((PROJ32, F32T, 128, 0, 0, 0, (128, 128)), False),
]


@pytest.mark.parametrize("key,served", THRESHOLDS, ids=[f"{k[0]}-{k[1]:#x}-{k[2]}-{k[3]}-{k[4]}-{k[5]}-{k[6][0]}x{k[6][1]}" for k, _ in THRESHOLDS])
def test_thresholds(lib, key, served):
    from founddiff_amd import _lib as L
    entry, opts, cin, cdw, cz, C_, (H, W) = key
    pl = L.pwdw_plan(lib, entry, opts, cin, {PROJ: 64, GRAM: 192}.get(entry, cdw), cz, C_, 1, H, W)
    assert (pl is not None) == served == bool(_ok(lib, entry, opts, cin, cdw, cz, C_, H, W)), (key, pl)


def test_nblk_queries_are_the_plan_grid(lib):
    from founddiff_amd import _lib as L
    shapes = [(c.H, c.W) for c in CASES] + SHAPES
    for H, W in shapes:
        for opts in (BF16, BF16 | LL):
            pl = L.pwdw_plan(lib, GRAM, opts, 64, 192, 0, 0, 2, H, W)
            if pl:
                assert pl["gx"] == lib.fd_pw_dw3x3_gram_nblk_opts(opts, H, W), (H, W, opts, pl)
                assert opts != BF16 or pl["gx"] == lib.fd_pw_dw3x3_gram_nblk(H, W)
        pl = L.pwdw_plan(lib, DWGRAM, BF16, 0, 0, 0, 64, 2, H, W)
        if pl:
            assert pl["gx"] == lib.fd_dwconv_gram_nblk(H, W), (H, W, pl)
        pl = L.pwdw_plan(lib, GRAM32, F32T, 64, 0, 0, 0, 2, H, W)
        if pl:
            assert pl["gx"] == lib.fd_pw_dw3x3_gram_f32_nblk(H, W), (H, W, pl)
    for c, pl in _plans(lib):
        nb = {GRAM: lambda: lib.fd_pw_dw3x3_gram_nblk_opts(pc.dtype_opts(c), c.H, c.W), DWGRAM: lambda: lib.fd_dwconv_gram_nblk(c.H, c.W),
              GRAM32: lambda: lib.fd_pw_dw3x3_gram_f32_nblk(c.H, c.W)}.get(c.entry)
        if nb:
            assert nb() == pl["gx"], (case_id(c), pl)


def test_fp32_entry_points_say_what_the_plan_refused(lib):
    """the argument check comes before anything touches a device: the message names the plan's reason, not a hand-written list"""
    from founddiff_amd import _lib as L

    def msg(name, *args):
        assert getattr(lib, name)(*args) != 0
        return lib.fd_last_error().decode()
    dw = lambda cin, cdw, H, W: msg("fd_pw_dw3x3_f32", None, 64, 0, cin, None, None, 1e-5, None, None, 128, None, None, cdw, None, None, 0, None,
                                    cdw, 0, 1, H, W, None)
    assert "W % 16" in dw(64, 64, 136, 152) and "16384" in dw(64, 64, 120, 128) and "Cdw" in dw(64, 160, 128, 128) and "Cin" in dw(128, 64, 128, 128)
    gr = lambda H, W: msg("fd_pw_dw3x3_gram_f32", None, 64, 0, 64, None, None, 1e-6, None, None, 128, None, None, None, 128, None, 1, H, W, None)
    assert "W % 8" in gr(128, 132) and "H % 8" in gr(132, 128) and "16384" in gr(120, 128)
    pj = lambda H, W: msg("fd_pw_dw3x3_proj_f32", None, 64, 0, 64, None, None, 1e-6, None, None, 128, None, None, None, 64, None, None, 64, None,
                          64, 0, 1, H, W, None)
    assert "W % 8" in pj(128, 132) and "16384" in pj(120, 128)
    del L


# ------------------------------------------------------------------------------------------------ the bound, checked on the CPU
TYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
_KEEP = {}


def _setup(lib, c, tname):
    """(operands, plan, {output: (reference, bound)}) of (case, 16-bit type) in fp64 on the CPU; the last one is kept"""
    key = (case_id(c), tname)
    if _KEEP.get("key") != key:
        tdt = TYPES[tname]
        rq = (lambda v: v) if pc.is32(c) else (lambda v: v.to(tdt).float())
        t, pl = pc.make_inputs(c, rq), pc.plan(lib, c)
        ref = pc.pwdw_reference(c, t, tdt, "cpu")
        _KEEP.clear()
        _KEEP.update(key=key, val=(t, pl, pc.error_bounds(c, t, ref, tdt, pl, "cpu"), rq))
    return _KEEP["val"]


def _types(c):
    return ("bf16",) if pc.is32(c) else ("bf16", "fp16")


@pytest.mark.parametrize("c,tname", [pytest.param(c, tn, id=f"{case_id(c)}-{tn}") for c in CASES for tn in _types(c)])
def test_restatement_stays_inside_the_bound(lib, c, tname):
    t, pl, eb, rq = _setup(lib, c, tname)
    got = pc.restate(c, t, TYPES[tname], pl)
    assert set(got) == set(eb)
    for k, (ref, bound) in eb.items():
        assert bool(torch.isfinite(bound).all()) and bool((bound >= 0).all()), k
        r, idx, e, b = pc.worst((got[k].double() - ref).abs(), bound)
        assert r <= 1.0, f"{case_id(c)}-{tname}: {k}: err / bound {r:.3f} at {idx}: |got - ref| = {e:.3e}, bound {b:.3e}"
    if c.entry != DWGRAM:
        assert pc.row_ratio(c, t) <= pc.RATIO_MAX, "an ordinary row with |mean| / std above RATIO_MAX"
        m = pc.measure_c_ln(c, rq)
        assert m <= pc.C_LN_MEASURED, f"{case_id(c)}-{tname}: the fp32 prologue is off by {m:.3e} abar: above C_LN_MEASURED"


# a case per kernel.  Where the launch stores per-pixel outputs any dense case shows a fault of one tile; the Gram partials (a bound summed
# over every pixel a workgroup walked) show it on the sparse cases.  fd_dwconv_gram has no 1x1, hence no weight group to take from the
# wrong place; in gram-v-exact the weight groups the fault mixes are q's (not stored): its v shows the other two
FAULT_CASES = ("dw64-128-128-b4-r3", "dw128-192-64-b1-r1", "proj-b1-exact", "gram-v-exact", "gram-sparse", "dwgram-sparse", "f32-64-b4-r2",
               "gram32-sparse", "proj32-b1-r3", "dw64-range-lo", "dw64-range-hi")
NO_GROUP_FAULT = ("gram-v-exact", "dwgram-sparse")


@pytest.mark.parametrize("c,fault", [pytest.param(c, f, id=f"{case_id(c)}-{f}") for c in CASES if c.name in FAULT_CASES for f in pc.FAULTS
                                     if not (f == "previous-group" and c.name in NO_GROUP_FAULT)])
def test_seeded_fault_leaves_the_bound(lib, c, fault):
    """one halo pixel from the clamped neighbour, one channel pair swapped, one tile's second weight group from the first: each in one
    tile of one image, each must show in the element-wise comparison of at least one output"""
    t, pl, eb, _ = _setup(lib, c, "bf16")
    got = pc.restate(c, t, torch.bfloat16, pl, fault=fault)
    worst = max(pc.worst((got[k].double() - ref).abs(), bound)[0] for k, (ref, bound) in eb.items())
    assert worst > 1.0, f"{case_id(c)}: the fault {fault} stays inside the bound (err / bound {worst:.3f}): the bound is too wide to see it"
