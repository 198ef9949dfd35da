"""fd_cross_scan_bwd_geom / fd_selective_scan_bwd_geom (host only): the two scan backwards' layouts as their launchers compute
them.  No GPU.

(1) tests/scan_bwd_cases.CS_CASES / SB_CASES, the shapes tests/test_gpu_scan_bwd_cases.py runs, reach every instantiation and
tiling edge of the two backwards -- asserted from the queries' answers, so a dropped case or a moved threshold names the edge that
lost its test -- and every case is needed: without any single one of them some edge is no longer reached.
(2) over the accepted domain, the workspace the library promises covers the regions the geometry implies, every launch grid fits
the hardware's limits and no kernel needs more than 64 KiB of LDS.
(3) the tables' inputs take both branches of softplus' derivative: delta + bias lies in 21 .. 25 on every 16th channel and far
below 20 on the others."""
import ctypes as C
import re

import pytest
import torch

import scan_bwd_cases as sc
from scan_bwd_cases import CS_CASES, SB_CASES, check_expected, cs_gaps, cs_geom, cs_id, sb_gaps, sb_geom, sb_id


@pytest.fixture(scope="module")
def lib():
    from founddiff_amd import _lib as L
    return L.lib()


def _cs_query(lib, B, H, W, D, N, R):
    out = (C.c_int32 * 8)()
    rc = lib.fd_cross_scan_bwd_geom(B, H, W, D, N, R, out)
    return rc, dict(zip(sc.CS_FIELDS, out))


def _sb_query(lib, batch, KD, K, N, L):
    out = (C.c_int32 * 8)()
    rc = lib.fd_selective_scan_bwd_geom(batch, KD, K, N, L, out)
    return rc, dict(zip(sc.SB_FIELDS, out))


def test_both_libraries_export_the_queries():
    from founddiff_amd import _lib as L
    for build in (L.BF16, L.F16):
        lib = build.lib()
        assert _cs_query(lib, 2, 63, 65, 128, 4, 4)[1] == dict(E=4, tile=256, L=1056, ntiles=5, last=32, S=2, nxb=5, lds=46784)
        assert _sb_query(lib, 1, 64, 2, 9, 257)[1] == dict(ntiles=2, tgroups=1, last=1, S=2, NC=8, rps=16, Dg=32)


def test_tables_are_well_formed(lib):
    for cases, ident in ((CS_CASES, cs_id), (SB_CASES, sb_id)):
        ids = [ident(c) for c in cases]
        assert len(ids) == len(set(ids)), "duplicate case"
    for c in CS_CASES:
        g = cs_geom(lib, c)
        check_expected(cs_id(c), c.expect, g)
        assert c.B in (1, 2)
        assert g["tile"] == 64 * g["E"] and g["ntiles"] == -(-g["L"] // g["tile"]) and 1 <= g["last"] <= g["tile"]
        assert g["E"] == (4 if c.R + 2 * c.N <= 24 else 1) and g["nxb"] == -(-g["L"] // 256)
    for c in SB_CASES:
        g = sb_geom(lib, c)
        check_expected(sb_id(c), c.expect, g)
        assert c.KD % (c.K * c.nrows) == 0, sb_id(c)
        assert g["ntiles"] == -(-c.L // 256) and g["tgroups"] == -(-g["ntiles"] // 4) and g["NC"] == (4 if c.N <= 4 else 8)
        assert g["Dg"] == c.KD // c.K and g["rps"] == -(-g["Dg"] // g["S"])


def test_cases_reach_every_edge(lib):
    assert cs_gaps([(c, cs_geom(lib, c)) for c in CS_CASES]) == []
    assert sb_gaps([(c, sb_geom(lib, c)) for c in SB_CASES]) == []


def test_every_case_is_needed(lib):
    """without any single case, the coverage test names at least one edge that lost its test"""
    for cases, geom, gaps, ident in ((CS_CASES, cs_geom, cs_gaps, cs_id), (SB_CASES, sb_geom, sb_gaps, sb_id)):
        rows = [(c, geom(lib, c)) for c in cases]
        for i, (c, _) in enumerate(rows):
            assert gaps(rows[:i] + rows[i + 1:]), f"{ident(c)} stands for no edge of its own"


def test_static_lds_is_the_compilers(lib):
    """out[7] of the cross-scan query against hipcc's own figure for the two kernels of every (N, R), in both builds"""
    from founddiff_amd import build as fb
    for half in ("bf16", "fp16"):
        tab = fb.resources(half)["fd_cross_scan_bwd.hip"]
        lds = {}
        for name, r in tab.items():
            m = re.search(r"cs_(scan|xproj)_kernelILi(\d+)ELi(\d+)E", name)
            if m:
                key = (int(m.group(2)), int(m.group(3)))
                lds[key] = max(lds.get(key, 0), r["lds"])
        assert len(lds) == 20, sorted(lds)
        for (N, R), v in lds.items():
            assert _cs_query(lib, 1, 16, 16, 64, N, R)[1]["lds"] == v, (half, N, R, v)


SWEEP_HW = (1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 600)
GRID_X, GRID_YZ = 2 ** 31 - 1, 65535


def _r4(n):
    return (n + 3) & ~3


def test_cross_scan_workspace_grids_and_lds(lib):
    """fd_cross_scan_bwd_ws_floats against the regions of csrc/fd_cross_scan_bwd.hip recomputed from the query's fields: three
    composite arrays [tile][B 4 D][N], the parameter partials [B tiles][4 D][N + R + 2], the dxdbl rows, their S split partials
    and the dx_proj_w partials [B nxb][4][CD][D]; the seven launch grids; the static LDS.  The grid of H, W and B is this
    sweep's own, not the library's limit: the library bounds one image by 2^31 bytes and B by 16383 (4 B is a grid.y), both
    asserted at their edges below."""
    for D in (64, 128, 256, 512, 1024):
        for N in (4, 8, 16, 32):
            for R in (2, 4, 8, 16, 32):
                CD = R + 2 * N
                for H in SWEEP_HW:
                    for W in SWEEP_HW:
                        for B in (1, 2, 16):
                            rc, g = _cs_query(lib, B, H, W, D, N, R)
                            ws = lib.fd_cross_scan_bwd_ws_floats(B, H, W, D, N, R)
                            if H * W * D * 4 >= 2 ** 31:
                                assert rc != 0 and ws == 0 and not any(g.values())
                                continue
                            assert rc == 0, (B, H, W, D, N, R)
                            L = ((H + 1) // 2) * ((W + 1) // 2)
                            assert g["L"] == L
                            rows = B * 4 * D
                            need = (3 * _r4(g["ntiles"] * rows * N) + _r4(B * g["ntiles"] * 4 * D * (N + R + 2)) + _r4(4 * B * L * CD)
                                    + (_r4(g["S"] * 4 * B * L * CD) if g["S"] > 1 else 0) + _r4(B * g["nxb"] * 4 * CD * D))
                            assert ws >= need, (B, H, W, D, N, R, g, ws, need)
                            assert g["S"] * 64 <= D and D % g["S"] == 0 and (D // g["S"]) % 16 == 0, g      # whole 16-channel slabs
                            grids = ((g["ntiles"] * g["S"], B * 4, 1), (-(-rows * N // 256), 1, 1), (-(-4 * B * L * CD // 256), 1, 1),
                                     (g["nxb"], B * 4, D // 64), (-(-4 * CD * D // 256), 1, 1), (-(-4 * D * (N + R + 2) // 256), 1, 1),
                                     (-(-H * W // 64), D // 64, B))
                            for x, y, z in grids:
                                assert 1 <= x <= GRID_X and 1 <= y <= GRID_YZ and 1 <= z <= GRID_YZ, (B, H, W, D, N, R, g)
                            assert g["lds"] <= 65536, g
    # the batch limit: batch x direction is grid.y of the scan and x_proj launches
    assert _cs_query(lib, 16383, 2, 2, 64, 4, 4)[0] == 0 and lib.fd_cross_scan_bwd_ws_floats(16383, 2, 2, 64, 4, 4) > 0
    assert _cs_query(lib, 16384, 2, 2, 64, 4, 4)[0] != 0 and lib.fd_cross_scan_bwd_ws_floats(16384, 2, 2, 64, 4, 4) == 0


def test_reference_layout_workspace_and_grids(lib):
    """fd_selective_scan_bwd_ws_floats against the regions of csrc/fd_scan_bwd.hip: three composite arrays [tile][batch KD][N], the
    parameter partials [N + 2][KD][batch][tile] and, with row splits, two sets of S dB / dC slabs; the five launch grids.  The
    sweep stops at 2^32 elements per activation (16 GiB in fp32); that bound is the sweep's, the library sets none.  The largest
    grid, batch KD ceil(L / 1024) carry workgroups, passes 2^31 only beyond 2^41 elements (8 TiB per activation)."""
    for batch in (1, 2, 16):
        for KD, K in ((4, 4), (24, 4), (24, 2), (64, 2), (90, 1), (96, 1), (128, 1), (512, 4), (4096, 4), (4096, 1)):
            for N in (1, 3, 4, 5, 8, 9, 16, 33, 256):
                for L in (1, 3, 255, 256, 257, 1023, 1024, 1025, 2049, 4096, 65536, 65537, 2 ** 20, 2 ** 24):
                    if batch * KD * L > 2 ** 32:
                        continue
                    rc, g = _sb_query(lib, batch, KD, K, N, L)
                    assert rc == 0, (batch, KD, K, N, L)
                    ws = lib.fd_selective_scan_bwd_ws_floats(batch, KD, K, N, L)
                    rows = batch * KD
                    need = (3 * _r4(g["ntiles"] * rows * N) + _r4((N + 2) * rows * g["ntiles"])
                            + (2 * _r4(g["S"] * batch * K * N * L) if g["S"] > 1 else 0))
                    assert ws >= need, (batch, KD, K, N, L, g, ws, need)
                    assert g["S"] == 1 or g["Dg"] // g["S"] >= 16, g
                    grids = (rows * g["tgroups"], -(-rows * N // 256), batch * K * g["S"] * g["ntiles"], KD,
                             -(-batch * K * N * L // 256))
                    assert all(1 <= x <= GRID_X for x in grids), (batch, KD, K, N, L, g, grids)


def test_queries_refuse_what_the_calls_refuse(lib):
    for args in ((2, 16, 16, 96, 4, 4), (2, 16, 16, 64, 6, 4), (2, 16, 16, 64, 4, 3), (0, 16, 16, 64, 4, 4), (2, 0, 16, 64, 4, 4),
                 (2, 16, 0, 64, 4, 4), (1, 1024, 1024, 512, 4, 4), (16384, 16, 16, 64, 4, 4)):
        rc, g = _cs_query(lib, *args)
        assert rc != 0 and not any(g.values()), args
        assert b"fd_cross_scan_bwd_geom" in lib.fd_last_error()
        assert lib.fd_cross_scan_bwd_ws_floats(*args) == 0
    for args in ((2, 510, 4, 4, 64), (0, 512, 4, 4, 64), (2, 512, 0, 4, 64), (2, 512, 4, 0, 64), (2, 512, 4, 257, 64),
                 (2, 512, 4, 4, 0)):
        rc, g = _sb_query(lib, *args)
        assert rc != 0 and not any(g.values()), args
        assert b"fd_selective_scan_bwd_geom" in lib.fd_last_error()
    assert lib.fd_cross_scan_bwd_geom(2, 16, 16, 64, 4, 4, None) != 0
    assert lib.fd_selective_scan_bwd_geom(2, 512, 4, 4, 64, None) != 0
    # H = 1 and W = 1 are served, as the forward serves them
    assert _cs_query(lib, 1, 1, 9, 64, 4, 4)[0] == 0 and _cs_query(lib, 1, 9, 1, 64, 4, 4)[0] == 0


def _branches(v, hot, tag):
    """v = delta + bias (float64) with the channel axis at dim -2"""
    cold = torch.ones(v.shape[-2], dtype=torch.bool)
    cold[hot] = False
    assert 21.0 < float(v[..., hot, :].min()) and float(v[..., hot, :].max()) < 25.0, (tag, float(v[..., hot, :].min()),
                                                                                      float(v[..., hot, :].max()))
    assert not cold.any() or float(v[..., cold, :].max()) < 15.0, (tag, float(v[..., cold, :].max()))


def test_inputs_take_both_softplus_branches():
    """the float64 reference's v = delta + bias: in 21 .. 25 on every 16th channel (softplus' derivative is 1 there, v > 20), below
    15 on every other one (the sigmoid branch), in every case that runs with softplus"""
    for c in CS_CASES:
        x, _, p = sc.cs_inputs(c)
        _, v = sc.cs_xdbl_rows(x.double(), {k: t.double() for k, t in p.items()})               # (B, 4, D, L)
        _branches(v, torch.arange(0, c.D, sc.HOT_EVERY), cs_id(c))
    for c in SB_CASES:
        u, delta, A, Bm, Cm, D, bias, dout = sc.sb_inputs(c)
        v = delta.double() + (bias.double()[None, :, None] if bias is not None else 0)
        if not c.softplus:                      # dt = v itself: a decaying state needs dt >= 0
            assert 0.0 <= float(v.min()) and float(v.max()) < 1.0, sb_id(c)
            continue
        _branches(v, torch.arange(0, c.KD, sc.HOT_EVERY), sb_id(c))
    assert sum(not c.softplus for c in SB_CASES) >= 3
