"""fd_gemm_rows_form (host only): which instantiation of the streaming row-GEMM fd_conv2d launches, and on which grid.  No GPU.

tests/rows_cases.rows_cases(), the shapes tests/test_gpu_rows_forms.py runs, reach every compiled form of gemm_rows_kernel and
gemm_rows32_kernel that the dispatcher can reach, the three reachable z-recompute kernels, every edge of the coverage list below and
every item of the tile-walk list -- asserted from the query's answers and the case fields.  The compiled forms (the fits_512 / fits_768
rules of csrc/fd_gemm_rows.hip) and the output widths at which the workgroup grows (the 50 KiB / 75 KiB steps of the LDS image) are
written out as literals here, so a dropped case or a moved threshold of the dispatcher names what lost its test."""
import os

import pytest
import torch

import rows_cases as rc
from rows_cases import EDGE_CASES, WALK_CASES, WALK_FAMILIES, case_id, form, kernel_of


@pytest.fixture(scope="module")
def lib():
    for var in ("FD_ROWS_PER_CU_MAX", "FD_ROWS_PER_CU", "FD_ROWS32_PER_CU", "FD_ZRE_NOPF"):
        assert var not in os.environ, (f"{var} is set: a development build of the library would plan other launches than the shipped "
                                       "one -- unset it")
    from founddiff_amd import _lib as L
    return L.lib()


ALL_NT = (256, 512, 768)
# 16-bit storage: KS -> the workgroup sizes compiled for it (csrc/fd_gemm_rows.hip: fits_512, fits_768), per prologue
NT_16 = {
    "NONE": {1: ALL_NT, 2: ALL_NT, 3: ALL_NT, 4: ALL_NT, 6: ALL_NT, 8: ALL_NT},
    "LN_MOD": {1: ALL_NT, 2: ALL_NT, 3: ALL_NT, 4: ALL_NT, 6: (256, 512), 8: (256,)},
    "LN_GATE": {1: ALL_NT, 2: ALL_NT, 3: ALL_NT, 4: (256, 512), 6: (256,), 8: (256,)},
}
# fp32 storage: 4- and 8-wave workgroups of every form (csrc/fd_gemm_rows32.hip)
NT_32 = {pro: {ks: (256, 512) for ks in rc.KS_ALL} for pro in NT_16}
# the z-recompute kernels of fd_gemm_rows_form's field [9]: 16-bit K = 128, 16-bit K = 256, fp32 storage K = 128
ZRE = {"bf16": (1, 2), "fp32s": (3,)}
# (mode, K) -> the widest Cout at NT 256, the narrowest at NT 512, the narrowest at NT 768 (no prologue, B = 1): the LDS steps
COUT_STEPS = {
    ("bf16", 32): (384, 416, 608), ("bf16", 64): (384, 416, 608), ("bf16", 96): (192, 224, 320), ("bf16", 128): (192, 224, 320),
    ("bf16", 192): (64, 96, 160), ("bf16", 256): (64, 96, 160),
    ("fp32s", 32): (288, 320, None), ("fp32s", 64): (288, 320, None), ("fp32s", 96): (128, 160, None), ("fp32s", 128): (128, 160, None),
    ("fp32s", 192): (64, 96, None), ("fp32s", 256): (64, 96, None),
}


def expected_kernels(mode):
    tab = NT_16 if mode == "bf16" else NT_32
    return ({(ks, pro, epi, nt) for pro, epi in rc.PAIRS for ks, nts in tab[pro].items() for nt in nts}
            | {("zre", z) for z in ZRE[mode]})


def _runs(lib):
    """(case, mode, plan) of every run of the GPU test's table"""
    return [(c, m, form(lib, c, m)) for c in rc.rows_cases(lib) for m in c.modes]


def _everything(lib):
    extra = (rc.BATCH_CASES + [rc.batch_slice(c, {}, 0)[0] for c in rc.BATCH_CASES] + [c for c, _ in rc.COLUMN_CASES]
             + [rc.column_slice(c, {"weight": torch.zeros(1, 1, c.cout, 1), "bias": torch.zeros(c.cout)}, 64)[0] for c, _ in rc.COLUMN_CASES]
             + [rc.COLS32_CASE])
    return _runs(lib) + [(c, m, form(lib, c, m)) for c in extra for m in c.modes]


# the hand-written cases the table was specified with: most items of the coverage lists are reached by more than one of them, so the
# coverage tests alone would let one go
MINIMUM_CASES = """cat-40+24 cat-72+56-relu silu-split-40 silu-split-72-k96 gn-groups-of-8 gn-groups-of-8-k128 lnmod-noaffine
lnmod-noaffine-k96-silu lnmod-special-k128 lngate-all-strided lngate-special-k64 wbatch-lnmod wbatch-lngate wbatch-gate-slice final-mode0
final-ddim final-ddim-last final-ddim-k32 s2-exact s2-one-row s2-half s2-half-lnmod s2-ragged-e s1-exact s1-one-row s1-ragged-e-k256
s1-one-row-lngate-k192 zre128-ragged zre128-exact-special zre128-one-row-noaffine-strided zre256-ragged zre256-exact-special
zre256-one-row-noaffine-strided walk-s2-one walk-s2-many walk-s2-many-lnmod walk-s1-256-one walk-s1-256-many walk-s1-512-one
walk-s1-512-many walk-s1-768-one walk-s1-768-many walk-zre128-many walk-zre256-many walk-rows32-512-one walk-rows32-512-many""".split()


def test_case_table_is_well_formed(lib):
    cases = rc.rows_cases(lib)
    ids = [case_id(c) for c in cases]
    assert len(ids) == len(set(ids)), "duplicate case"
    assert set(MINIMUM_CASES) <= set(ids), "dropped: " + " ".join(sorted(set(MINIMUM_CASES) - set(ids)))
    assert {case_id(c) for c in EDGE_CASES + WALK_CASES} <= set(ids)
    assert len(rc.BATCH_CASES) >= 6 and len(rc.COLUMN_CASES) >= 6
    for c in cases + rc.BATCH_CASES + [c for c, _ in rc.COLUMN_CASES] + [rc.COLS32_CASE]:
        n = case_id(c)
        assert set(c.modes) <= set(rc.MODES) and c.modes, n
        assert 16384 <= rc.npx(c) <= 33 * 1024 and c.B <= 4, n
        c0 = c.cin - c.c1
        for v in (c0, c.c1, c.ld0, c.off0, c.ld1, c.off1, c.ldo, c.offo, c.ld_res, c.off_res, c.ldz, c.offz, c.split):
            assert v % 8 == 0, (n, v)
        assert c.gate_ld % 4 == 0 and c.cout % 32 == 0, n
        assert c.off0 + c0 <= c.ld0 and c.off1 + c.c1 <= c.ld1 and c.offo + c.cout <= c.ldo and c.offz + c.cin <= c.ldz, n
        assert c.off_res + c.cout <= c.ld_res and c.cout <= c.gate_ld, n
        assert c.ln_ld >= (c.cin if c.pro in ("LN_GATE", "ZRE") else 2 * c.cin), n
        if c.epi in ("GNSILU_ADD", "GNSILU_ADD_FINAL"):
            assert c.groups > 0 and c.cout % c.groups == 0 and (c.cout // c.groups) % 8 == 0, n


def test_no_case_falls_off_the_row_gemm(lib):
    """fd_conv_kernel_id is 10 (16-bit storage) or 17 (fp32 storage) for every launch of the GPU module, and the plan says the same"""
    import ctypes as C
    for c, m, f in _everything(lib):
        p = rc.params_for(c, m, rc.DUMMY_PTRS)
        kid = lib.fd_conv_kernel_id(C.byref(p))
        assert kid == rc.KID[m], (case_id(c), m, f"runs on kernel {kid}, not on the row-GEMM")
        assert f is not None and f["kid"] == kid, (case_id(c), m, f)
        assert f["KS"] == c.cin // 32 and f["PRO"] == rc.PROS.index(c.pro) and f["EPI"] == rc.EPIS.index(c.epi), (case_id(c), m, f)
        assert f["S"] == (2 if m == "bf16" and c.cin <= 64 and c.pro != "ZRE" else 1), (case_id(c), m, f)
        assert f["wtiles"] == -(-rc.npx(c) // (16 * f["S"])) and 1 <= f["gx"] <= -(-f["wtiles"] // (f["NT"] // 64)), (case_id(c), m, f)
        assert 0 < f["lds"] <= 160 * 1024, (case_id(c), m, f)


def test_query_refuses_what_the_row_gemm_does_not_run(lib):
    c = rc._r("small", 1, (64, 64), 64, 64)            # below 16384 pixels: the tiled kernels
    assert form(lib, c, "bf16") is None and form(lib, c, "fp32s") is None
    c = rc._r("k160", 1, rc.TALL, 160, 64)             # no KS = 5 instantiation
    assert form(lib, c, "bf16") is None and form(lib, c, "fp32s") is None


@pytest.mark.parametrize("mode", rc.MODES)
def test_cases_reach_every_kernel(lib, mode):
    """every compiled form the dispatcher can reach is launched by a case -- and the table launches no form this list does not name"""
    reached = {}
    for c, m, f in _runs(lib):
        if m == mode:
            reached.setdefault(kernel_of(f), []).append(case_id(c))
    want = expected_kernels(mode)
    assert len(want) == {"bf16": 169 + 2, "fp32s": 120 + 1}[mode]
    lost = sorted(want - set(reached), key=str)
    assert not lost, f"[{mode}] no case of tests/rows_cases reaches (KS, PRO, EPI, NT): " + "; ".join(map(str, lost))
    new = sorted(set(reached) - want, key=str)
    assert not new, f"[{mode}] launched but not in the expected list (a fits_* rule moved?): " + "; ".join(f"{k} by {reached[k][0]}" for k in new)


def test_lds_steps_are_where_the_table_was_built(lib):
    """the widths at which the plan moves from 4 to 8 to 12 waves per workgroup: every (mode, K), and K = 32 width by width"""
    moved = []
    for (mode, K), (w256, n512, n768) in COUT_STEPS.items():
        got = {}
        for co in range(32, 1025, 32):
            f = form(lib, rc._r("x", 1, rc.TALL, K, co), mode)
            if f is not None:
                got.setdefault(f["NT"], []).append(co)
        have = (max(got[256]), min(got.get(512, [None])), min(got.get(768, [None])))
        if have != (w256, n512, n768):
            moved.append(f"{mode} K = {K}: (widest NT 256, narrowest NT 512, narrowest NT 768) = {have}, the table was built for {(w256, n512, n768)}")
    assert not moved, "the LDS steps of the plan moved: " + "; ".join(moved)
    nt = lambda mode, K, co: form(lib, rc._r("x", 1, rc.TALL, K, co), mode)["NT"]
    assert [nt("bf16", 32, co) for co in (32, 384, 416, 576, 608, 1024)] == [256, 256, 512, 512, 768, 768]


def features(c, m, f):
    """the items of the coverage list that (case, mode) reaches under the plan f"""
    s = set()
    hw, S = rc.npx(c), f["S"]
    r = hw % (16 * S)
    s.add(f"M S={S}: " + ("last tile full" if r == 0 else "last tile holds one row" if r == 1 else "last tile ragged"))
    if S == 2 and 0 < r <= 16:
        s.add("M S=2: second subtile empty")
    if S == 2 and r == 16:
        s.add("M S=2: first subtile full, second empty")
    if c.cout == 32:
        s.add("N: Cout 32")
    if c.c1 and (c.cin - c.c1) % 32:
        s.add("K: c0 inside a 32-channel step")
    if c.epi == "SILU_SPLIT" and c.split % 32:
        s.add("epi: SILU_SPLIT split % 32 != 0")
    if c.epi in ("GNSILU_ADD", "GNSILU_ADD_FINAL") and c.cout // c.groups == 8:
        s.add("epi: GroupNorm groups of 8 channels")
    if c.epi == "GNSILU_ADD_FINAL":
        s.add(f"epi: final, fin_mode {c.fin_mode} fin_last {c.fin_last}")
    if c.pro == "LN_MOD" and not c.affine:
        s.add("pro: LN_MOD without gamma / beta")
    if c.pro == "ZRE" and not c.affine:
        s.add(f"pro: zre {f['zre']} norm1 without gamma / beta")
    if (c.pro == "LN_GATE" and c.ldz > c.cin and c.offz and c.gate_ld > c.cout and c.ld_res > c.cout and c.off_res and c.ldo > c.cout
            and c.offo and c.ld0 > c.cin and c.off0 and c.ln_ld > c.cin):
        s.add("strides: ln_ldz / ln_offz, gate_ld, ld_res / off_res, ldo / offo, ld0 / off0 at once")
    if c.wb and c.pro != "NONE":
        s.add(f"src: per-image weights with {c.pro}")
    if c.special:
        s.add(f"pro: zero-variance and zero rows under {c.pro}" + (f" {f['zre']}" if c.pro == "ZRE" else ""))
    if c.pro == "ZRE":
        s.add(f"zre {f['zre']}: " + ("exact" if hw % 16 == 0 else "ragged"))
    return s


ANY, H16, F32 = rc.MODES, ("bf16",), ("fp32s",)
REQUIRED = (
    [(f"M S=2: {x}", H16) for x in ("last tile full", "last tile holds one row", "last tile ragged", "second subtile empty",
                                    "first subtile full, second empty")]
    + [(f"M S=1: {x}", ANY) for x in ("last tile full", "last tile holds one row", "last tile ragged")]
    + [(x, ANY) for x in ("N: Cout 32", "K: c0 inside a 32-channel step", "epi: SILU_SPLIT split % 32 != 0",
                          "epi: GroupNorm groups of 8 channels", "epi: final, fin_mode 0 fin_last 0", "epi: final, fin_mode 1 fin_last 0",
                          "epi: final, fin_mode 1 fin_last 1", "pro: LN_MOD without gamma / beta",
                          "strides: ln_ldz / ln_offz, gate_ld, ld_res / off_res, ldo / offo, ld0 / off0 at once",
                          "src: per-image weights with LN_MOD", "src: per-image weights with LN_GATE",
                          "pro: zero-variance and zero rows under LN_MOD", "pro: zero-variance and zero rows under LN_GATE")]
    + [(x, H16) for z in (1, 2) for x in (f"zre {z}: exact", f"zre {z}: ragged", f"pro: zero-variance and zero rows under ZRE {z}",
                                          f"pro: zre {z} norm1 without gamma / beta")]
    + [(x, F32) for x in ("zre 3: exact", "zre 3: ragged", "pro: zero-variance and zero rows under ZRE 3",
                          "pro: zre 3 norm1 without gamma / beta")]
)


def test_cases_reach_every_edge(lib):
    reached = {}
    for c, m, f in _runs(lib):
        for item in features(c, m, f):
            reached.setdefault(item, {}).setdefault(m, []).append(case_id(c))
    lost = [f"{item} [{m}]" for item, modes in REQUIRED for m in modes if not reached.get(item, {}).get(m)]
    assert not lost, "no case of tests/rows_cases reaches: " + "; ".join(lost)


# family -> what the plan of its two cases must say: (S, NT, z-recompute kernel, kernel id)
WALK_KERNELS = {"generic S=2": (2, 256, 0, 10), "generic S=1 NT 256": (1, 256, 0, 10), "generic S=1 NT 512": (1, 512, 0, 10),
                "generic S=1 NT 768": (1, 768, 0, 10), "zre K=128": (1, 256, 1, 10), "zre K=256": (1, 512, 2, 10),
                "rows32 NT 256": (1, 256, 0, 17), "rows32 NT 512": (1, 512, 0, 17), "rows32 zre": (1, 256, 3, 17)}


def test_cases_walk_the_tiles(lib):
    """each kernel family once with a wave per tile and once with waves that walk at least two tiles and a ragged last round"""
    by_name = {case_id(c): c for c in rc.rows_cases(lib)}
    assert set(WALK_FAMILIES) == set(WALK_KERNELS)
    lost = []
    for fam, (one, many) in WALK_FAMILIES.items():
        for kind, (name, m) in (("one", one), ("many", many)):
            if name not in by_name or m not in by_name[name].modes:
                lost.append(f"{fam}: the case {name} [{m}] is gone")
                continue
            f = form(lib, by_name[name], m)
            if (f["S"], f["NT"], f["zre"], f["kid"]) != WALK_KERNELS[fam]:
                lost.append(f"{fam}: {name} [{m}] runs (S, NT, zre, kid) = {(f['S'], f['NT'], f['zre'], f['kid'])}")
                continue
            waves, need = f["gx"] * f["NT"] // 64, -(-f["wtiles"] // (f["NT"] // 64))
            if kind == "one" and f["gx"] != need:
                lost.append(f"{fam}: {name} [{m}] has grid x {f['gx']} != need {need}: its waves walk")
            if kind == "many" and not (f["gx"] < need and f["wtiles"] > waves and f["wtiles"] % waves != 0):
                lost.append(f"{fam}: {name} [{m}] walks no ragged second round: wtiles {f['wtiles']}, {waves} waves")
    assert not lost, "; ".join(lost)


def test_bit_for_bit_cases_move_what_they_claim(lib):
    """batch invariance: B = 4 against B = 1 changes the grid (and the workgroups-per-CU limit); column invariance: NT 512 / 768 against 256"""
    for c in rc.BATCH_CASES:
        for m in c.modes:
            f4, f1 = form(lib, c, m), form(lib, rc.batch_slice(c, {}, 0)[0], m)
            assert kernel_of(f4) == kernel_of(f1) and f4["gx"] != f1["gx"], (case_id(c), m, f4, f1)
            assert f4["wtiles"] > f4["gx"] * f4["NT"] // 64 and f1["wtiles"] <= f1["gx"] * f1["NT"] // 64, (case_id(c), m, f4, f1)
    for c, nt in rc.COLUMN_CASES:
        narrow = rc.column_slice(c, {"weight": torch.zeros(1, 1, c.cout, 1), "bias": torch.zeros(c.cout)}, 64)[0]
        assert form(lib, c, "bf16")["NT"] == nt and form(lib, narrow, "bf16")["NT"] == 256, case_id(c)
    c = rc.COLS32_CASE
    assert form(lib, c, "fp32s")["NT"] == 256 and form(lib, c._replace(cout=c.cout // 2, ldo=c.cout), "fp32s") is not None


def test_engine_probe_rows(lib):
    """DAEngine.conv(probe="rows") poses the same question"""
    from founddiff_amd import _lib as L
    from founddiff_amd.engine import _T, DAEngine

    class Bare(DAEngine):
        def __init__(self, mode):
            self.mode, self.hip, self.dev, self.buf = mode, L.BF16, torch.device("cpu"), {}
            self.dt, self.tdt = _T[mode]
            self.f32_split = int(mode == "fp32s")
    by_name = {case_id(c): c for c in rc.rows_cases(lib)}
    for name in ("walk-s1-768-many", "lngate-all-strided", "s2-half", "walk-rows32-512-one"):
        c = by_name[name]
        for m in c.modes:
            e = Bare(m)
            z, zf = torch.zeros(16, dtype=e.tdt), torch.zeros(16)
            kw = dict(c0=c.cin, ld0=c.ld0, off0=c.off0, weight=z, bias=zf if c.bias else None, Cout=c.cout, KH=1, KW=1,
                      epi=rc.EPIS.index(c.epi), res=z if c.epi in ("GATE_RES", "RES_RELU") else None, ldo=c.ldo, offo=c.offo,
                      ld_res=c.ld_res, off_res=c.off_res, gate=zf if c.epi == "GATE_RES" else None, gate_ld=c.gate_ld,
                      prologue=rc.PROS.index(c.pro))
            if c.pro != "NONE":
                kw.update(ln_gamma=zf, ln_beta=zf, ln_shift=zf, ln_scale=zf if c.pro == "LN_MOD" else None, ln_ld=c.ln_ld)
            if c.pro == "LN_GATE":
                kw.update(ln_z=z, ln_ldz=c.ldz, ln_offz=c.offz)
            got = e.conv(None, z, c.B, c.H, c.W, z, probe="rows", **kw)
            assert got == form(lib, c, m) and got["kid"] == rc.KID[m], (name, m, got)
            assert e.conv(None, z, c.B, c.H, c.W, z, probe="kid", **kw) == rc.KID[m]
    assert Bare("bf16").conv(None, torch.zeros(16), 1, 16, 16, torch.zeros(16), probe="rows", c0=64, weight=torch.zeros(16), bias=None,
                             Cout=64, KH=1, KW=1) is None


def test_c_ln_is_what_the_reference_measures():
    """rows_cases.C_LN_MEASURED is the fp32-torch-against-fp64 figure of the table's own inputs (its worst case and two ordinary ones
    here; the whole table takes 20 s), and the bound uses 4 x that"""
    rq = {"bf16": lambda t: t.to(torch.bfloat16).float(), "fp32s": lambda t: t}
    by_name = {case_id(c): c for c in EDGE_CASES}
    worst = rc.measure_c_ln(by_name[rc.C_LN_WORST[0]], rq[rc.C_LN_WORST[1]])
    assert 0.5 * rc.C_LN_MEASURED <= worst <= 1.25 * rc.C_LN_MEASURED, worst
    for name, m in (("lnmod-noaffine", "bf16"), ("lngate-special-k64", "fp32s")):
        assert rc.measure_c_ln(by_name[name], rq[m]) <= rc.C_LN_MEASURED, name
    assert rc.C_LN == 4 * rc.C_LN_MEASURED
