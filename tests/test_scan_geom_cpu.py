"""fd_selective_scan_geom (host only): the launcher's decisions as the launcher itself makes them.  No GPU.

(1) tests/scan_cases.SCAN_CASES, the shapes tests/test_gpu_scan_forms.py runs, reach every form of the scan's dispatch --
asserted from the query's answers, so a dropped case or a moved threshold names the form that lost its test.
(2) the workspace size fd_scan_ws_floats promises covers both kernel sets, and no accepted shape needs more than 64 KiB of
dynamic LDS."""
import ctypes as C

import pytest

import scan_cases as sc
from scan_cases import BATCH_CASES, SCAN_CASES, case_id, check_expected, geom


@pytest.fixture(scope="module")
def lib():
    from founddiff_amd import _lib as L
    return L.lib()


def _rows(lib):
    """(case, mode, geometry) of every run of the GPU test"""
    return [(c, m, geom(lib, c, m)) for c in SCAN_CASES for m in c.modes]


# the shapes the table was specified with: several forms are reached by more than one of them, so the coverage test alone would let
# one go (the combination it stands for -- chunked N = 16 on an odd image through <8>, say -- is reached by no other single case)
MINIMUM_CASES = """64-16-8-91x93 128-4-4-92x92 128-4-4-182x181 512-16-16-66x66 512-32-16-66x64 1024-4-2-182x182-b1 1024-32-32-182x182-b1
1024-4-2-256x256-b1 64-4-4-128x64 64-4-4-66x126 64-4-4-256x128 64-4-4-172x192 128-8-4-158x2 128-8-4-160x2 128-8-4-162x2 64-16-8-78x2-ll
64-16-8-80x2-ll 64-16-8-82x2-ll 128-16-8-2x2 128-16-8-62x2 128-16-8-64x2 128-16-8-66x2 128-16-8-66x62 128-16-8-63x61 128-16-8-63x63
1024-32-32-34x30-ll 128-4-4-130x130-ll 128-4-4-92x93-xproj 256-8-8-183x182-xproj 256-16-8-66x66-xproj 256-16-8-32x32-ll-xproj
256-8-8-66x66-xproj""".split()


def test_case_table_is_well_formed(lib):
    ids = [case_id(c) for c in SCAN_CASES]
    assert len(ids) == len(set(ids)), "duplicate case"
    assert set(MINIMUM_CASES) <= set(ids), sorted(set(MINIMUM_CASES) - set(ids))
    modes = {case_id(c): set(c.modes) for c in SCAN_CASES}
    assert all(modes[i] == {"fp32", "bf16"} for i in MINIMUM_CASES if "xproj" not in i)
    assert modes["128-4-4-92x93-xproj"] == {"bf16", "fp32s"} and modes["256-8-8-66x66-xproj"] == {"fp32s"}
    for c in SCAN_CASES:
        assert set(c.modes) <= ({"bf16", "fp32s"} if c.fused else {"fp32", "bf16"}), case_id(c)
        assert c.B in (1, 2)
        for m in c.modes:
            if c.fused:        # the engine's own precondition for fd_selective_scan_xproj
                assert lib.fd_selective_scan_fuses_xproj(sc.dtype_opts(c, m) & ~sc.LOW_LATENCY, c.D, c.N, c.R) == 1, (case_id(c), m)
            check_expected(c, m, geom(lib, c, m))
    for c, m in BATCH_CASES:
        check_expected(c, m, geom(lib, c, m))


def test_geom_matches_the_plan_query(lib):
    """the two host queries agree on the single-pass form, and the geometry does not depend on what the other call computes"""
    for c, m, g in _rows(lib):
        if not c.fused:
            seq = g["form"] == 0
            assert seq == (not c.ll and seq_ok(c)), (case_id(c), m)
            if lib.fd_selective_scan_fuses_xproj(sc.dtype_opts(c, m) & ~sc.LOW_LATENCY, c.D, c.N, c.R):
                assert lib.fd_selective_scan_plan(sc.dtype_opts(c, m), c.D, c.N, c.R, c.H, c.W) == (0 if seq else 1)
        if g["form"] == 0:
            assert all(g[k] == 0 for k in sc.GEOM_FIELDS), g
        else:
            assert g["nch"] == -(-g["L"] // g["cl"]) and 1 <= g["last"] <= g["cl"]
            assert c.D == 64 * g["cpl"] * g["nw"] * g["wgs"]


def seq_ok(c):
    """the single-pass form's documented domain (include/founddiff_hip.h): L <= 1024, N >= 16, R % 8 == 0"""
    return sc.seq_len(c) <= 1024 and c.N >= 16 and c.R % 8 == 0


def _reached(rows, key, pred=lambda c, m, g: True):
    return {key(c, m, g) for c, m, g in rows if pred(c, m, g)}


def test_cases_reach_every_form(lib):
    rows = _rows(lib)
    chunked = lambda c, m, g: g["form"] == 1
    h16 = lambda c, m, g: m == "bf16"
    f32 = lambda c, m, g: m == "fp32"
    both = lambda p, q: (lambda c, m, g: p(c, m, g) and q(c, m, g))
    plain = lambda c, m, g: not c.fused
    for name, typ in (("fp32", f32), ("16-bit", h16)):
        t = both(typ, plain)
        tc = both(t, chunked)
        assert _reached(rows, lambda c, m, g: g["form"], t) == {0, 1}, name
        # chunk length: 32 in the low-latency set only
        assert _reached(rows, lambda c, m, g: g["cl"], tc) == {32, 64, 128, 256}, name
        assert _reached(rows, lambda c, m, g: c.ll, both(tc, lambda c, m, g: g["cl"] == 32)) == {True}, name
        assert _reached(rows, lambda c, m, g: g["carry"], tc) == {-1, 2, 8, 0}, name
        # both sides of the carry kernels' boundaries
        assert {32, 33, 128, 129} <= _reached(rows, lambda c, m, g: g["nch"], tc), name
        for nch, carry in ((32, 2), (33, 8), (128, 8), (129, 0)):
            assert (nch, carry) in _reached(rows, lambda c, m, g: (g["nch"], g["carry"]), tc), (name, nch, carry)
        assert _reached(rows, lambda c, m, g: g["nw"], tc) == {1, 2, 4}, name
        assert _reached(rows, lambda c, m, g: min(g["wgs"], 2), tc) == {1, 2}, name
        assert _reached(rows, lambda c, m, g: (c.H | c.W) & 1, tc) == {0, 1}, name
        assert _reached(rows, lambda c, m, g: (c.H | c.W) & 1, both(t, lambda c, m, g: g["form"] == 0)) == {0, 1}, name
        assert _reached(rows, lambda c, m, g: c.N, tc) == {4, 8, 16, 32}, name
        assert _reached(rows, lambda c, m, g: c.R, tc) == {2, 4, 8, 16, 32}, name
        # the last chunk around the group length U of the chunk kernel's prefetch groups: 16 for N < 16, 8 from N = 16
        for U, pu in ((16, lambda c, m, g: c.N < 16), (8, lambda c, m, g: c.N >= 16)):
            got = _reached(rows, lambda c, m, g: g["last"] % g["cl"], both(tc, pu))
            assert {0, 1, U - 1, U, U + 1} <= got, (name, U, sorted(got))
            assert True in _reached(rows, lambda c, m, g: g["last"] == g["cl"] - 1, both(tc, pu)), (name, U)
        assert {1, 31, 32, 33, 1023, 1024} <= _reached(rows, lambda c, m, g: g["L"], both(t, lambda c, m, g: g["form"] == 0)), name
        # the low-latency set: no single-pass form, 32-step chunks where the image is small, one channel per lane
        ll = both(t, lambda c, m, g: c.ll)
        assert _reached(rows, lambda c, m, g: g["form"], ll) == {1} and _reached(rows, lambda c, m, g: g["cpl"], ll) == {1}, name
        assert True in _reached(rows, lambda c, m, g: seq_ok(c), ll), name          # a shape the other set runs single-pass
    # channels per lane: two is 16-bit only
    assert _reached(rows, lambda c, m, g: g["cpl"], both(both(h16, plain), chunked)) == {1, 2}
    assert _reached(rows, lambda c, m, g: g["cpl"], both(lambda c, m, g: m != "bf16", chunked)) == {1}
    # x_proj inside phase A
    fused = lambda c, m, g: c.fused
    assert _reached(rows, lambda c, m, g: (g["cpl"], c.ll), both(fused, h16)) == {(2, False), (1, False), (1, True)}
    assert 128 in _reached(rows, lambda c, m, g: c.D, both(fused, lambda c, m, g: g["cpl"] == 2))
    assert _reached(rows, lambda c, m, g: g["form"], fused) == {1}
    assert len(_reached(rows, lambda c, m, g: case_id(c), both(fused, lambda c, m, g: m == "fp32s"))) >= 2
    assert _reached(rows, lambda c, m, g: g["carry"], both(fused, h16)) >= {8, 0}


SWEEP_HW = [(2, 2), (3, 5), (8, 8), (15, 24), (16, 37), (31, 33), (32, 32), (33, 31), (62, 66), (63, 65), (64, 64), (65, 63), (66, 62),
            (91, 93), (92, 92), (127, 129), (128, 64), (128, 128), (129, 127), (130, 130), (172, 192), (181, 182), (183, 182), (255, 257),
            (256, 128), (256, 256), (257, 255), (300, 200), (362, 363), (511, 513), (512, 512), (513, 511), (640, 480), (724, 724),
            (1023, 1025), (1024, 1024)]


def _query(lib, opts, fused, D, N, R, H, W):
    out = (C.c_int32 * 8)()
    rc = lib.fd_selective_scan_geom(opts, fused, D, N, R, H, W, out)
    return rc, dict(zip(sc.GEOM_FIELDS, out))


def test_workspace_and_lds_bounds(lib):
    """fd_scan_ws_floats is sized by the low-latency geometry and claims to bound both kernel sets: 2 B 4 nch N D floats of chunk
    states (the sums of dt, B 4 nch D, fit in the second half).  Every shape the library accepts stays within 64 KiB of LDS; what
    would not (N = 32 in 256-step chunks: 68 KiB with R = 2, 96 KiB with R = 32) is refused, by the query and by the call."""
    refused = []
    for D in (64, 128, 256, 512, 1024):
        for N in (4, 8, 16, 32):
            for H, W in SWEEP_HW:
                if H * W * D * 4 >= 2 ** 31:
                    assert _query(lib, sc.FD_F32, 0, D, N, 4, H, W)[0] != 0
                    continue
                for B in (1, 3):
                    ws = lib.fd_scan_ws_floats(B, H, W, D, N)
                    for opts in (sc.FD_F32, sc.FD_BF16, sc.FD_F32 | sc.LOW_LATENCY, sc.FD_BF16 | sc.LOW_LATENCY):
                        for R in (2, 32):
                            rc, g = _query(lib, opts, 0, D, N, R, H, W)
                            if g["form"] == 0:
                                assert rc == 0
                                continue
                            need = 2 * B * 4 * g["nch"] * N * D
                            assert need <= ws, (B, D, N, R, H, W, opts, g, ws)
                            cd = (R + 2 * N + 3) & ~3
                            assert g["lds"] == g["cl"] * cd * 4, g
                            if rc != 0:
                                assert g["lds"] > 65536, (D, N, R, H, W, opts, g)
                                assert b"LDS" in lib.fd_last_error()
                                refused.append((D, N, R, g["cl"]))
                            else:
                                assert g["lds"] <= 65536, (D, N, R, H, W, opts, g)
    # only the widest state in the longest chunks: 256 rows of 68 (R = 2) .. 96 (R = 32) floats
    assert {(n, r, cl) for _, n, r, cl in refused} == {(32, 2, 256), (32, 32, 256)}, set(refused)
    # fused x_proj (d_inner <= 256): + 4 KiB for the two-channel form's u block, still far below the limit
    for D in (64, 128, 256):
        for N, R in ((4, 4), (8, 8), (16, 8), (32, 32)):
            for H, W in SWEEP_HW:
                for opts in (sc.FD_BF16, sc.FD_BF16 | sc.LOW_LATENCY, sc.FD_F32 | sc.F32_SPLIT):
                    if not lib.fd_selective_scan_fuses_xproj(opts & ~sc.LOW_LATENCY, D, N, R):
                        assert _query(lib, opts, 1, D, N, R, H, W)[0] != 0
                        continue
                    rc, g = _query(lib, opts, 1, D, N, R, H, W)
                    assert g["form"] == 1 and (rc == 0) == (g["lds"] <= 65536), (D, N, R, H, W, opts, g)
                    assert 2 * 4 * g["nch"] * N * D <= lib.fd_scan_ws_floats(1, H, W, D, N)


def test_oversized_lds_is_refused_by_the_call(lib):
    """d_inner 1024, N = 32, R = 32 at 256 x 256: L = 16384, 256-step chunks of 96-float rows = 96 KiB.  The query refuses it, and
    so does fd_selective_scan itself, before it touches a pointer or the device (the buffers here are a few host bytes)."""
    from founddiff_amd import _lib as L
    D, N, R, H, W = 1024, 32, 32, 256, 256
    for opts in (sc.FD_F32, sc.FD_BF16):
        rc, g = _query(lib, opts, 0, D, N, R, H, W)
        assert rc != 0 and g["cl"] == 256 and g["lds"] == 256 * 96 * 4
        assert b"LDS" in lib.fd_last_error()
        # (only after the query -- the same host function -- has refused: the call below must never reach a launch)
        buf = (C.c_float * 64)()
        p = C.addressof(buf)
        with pytest.raises(L.FoundDiffHipError, match="LDS"):
            L.call("fd_selective_scan", opts, p, p, p, p, p, p, p, p, 1, H, W, D, N, R, None)
    # the low-latency set runs this shape in 256-step chunks too (the chunk length only shrinks for small images)
    assert _query(lib, sc.FD_BF16 | sc.LOW_LATENCY, 0, D, N, R, H, W)[0] != 0
    # one size down it is served: 128-step chunks, 48 KiB
    rc, g = _query(lib, sc.FD_BF16, 0, D, N, R, 182, 182)
    assert rc == 0 and g["lds"] == 49152


def test_geom_refuses_what_the_call_refuses(lib):
    for args in ((sc.FD_F32, 0, 96, 4, 4, 16, 16), (sc.FD_F32, 0, 64, 6, 4, 16, 16), (sc.FD_F32, 0, 64, 4, 3, 16, 16),
                 (sc.FD_F32, 0, 64, 4, 4, 0, 16), (sc.FD_F32, 1, 128, 4, 4, 16, 16), (sc.FD_BF16, 1, 512, 32, 16, 16, 16)):
        rc, g = _query(lib, *args)
        assert rc != 0 and not any(g.values()), args
    assert lib.fd_selective_scan_geom(sc.FD_F32, 0, 64, 4, 4, 16, 16, None) != 0
