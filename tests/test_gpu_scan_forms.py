"""Every dispatch form of fd_selective_scan / fd_selective_scan_xproj against an fp64 scan.

The cases are tests/scan_cases.SCAN_CASES (tests/test_scan_geom_cpu.py asserts, without a GPU, that they reach every form: single-pass
and chunked, chunk lengths 32 .. 256, one and two channels per lane, 1 / 2 / 4 waves, several workgroups per chunk, every carry
kernel and the memset, odd images, last chunks of every awkward length, x_proj inside phase A in bf16 and split fp32, both kernel
sets).  The reference is oracle.nets.selective_scan_f64 on explicitly gathered operands (scan_cases.scan_reference).

Gates.  fp32 against fp64: 1e-5 max-rel, the gate of the 65 536-step test (the sequential fp32 CPU oracle is itself 0.8-2.0e-7
from fp64 at the largest shapes).  Split-fp32 fused: 1e-4 for the x_dbl rows and for y (the fp32s gate of test_conv).  16-bit:
conftest.gate2x, 2 x the error recorded on an MI355X (tests/golden/bf16_measured_errors.json), blanket 1e-2; inputs pre-rounded to
the build's 16-bit type.  bf16 fused x_dbl rows: 1e-5.

Beyond the comparison, on every case: y (and the fused x_dbl) is pre-filled with NaN and comes back finite; the workspace is exactly
fd_scan_ws_floats long, pre-filled with NaN, and a 64-float guard behind it and a guard row behind y stay untouched -- the kernels
neither read stale workspace nor write past either buffer."""
import pytest
import torch

import scan_cases as sc
from conftest import HB, gate2x, rel_err, use_half_build
from scan_cases import BATCH_CASES, SCAN_CASES, case_id, check_expected, geom, scan_reference

pytestmark = pytest.mark.gpu

GUARD = 64                    # floats behind the workspace
SENTINEL = -12345.0           # exact in fp32, bf16 rounds it to a finite value: the guards are compared with their own bits


@pytest.fixture(scope="module", params=["bf16-build", "fp16-build"], autouse=True)
def half_build(request):
    """every test of this module once per build of the library (conftest.use_half_build)"""
    use_half_build(request.param == "fp16-build")
    yield request.param
    use_half_build(False)


@pytest.fixture(autouse=True)
def _default_build_only(request, half_build):
    """the fp32-storage and split modes belong to the default build: not repeated on the binary16 one"""
    if half_build == "fp16-build":
        mode = getattr(request.node, "callspec", None) and request.node.callspec.params.get("mode")
        if mode in ("fp32", "fp32s"):
            pytest.skip("default build only")


def _inputs(c, B, mode, seed=5):
    """operands of one call, on the CPU in fp32: test_selective_scan's recipe.  16-bit: xc and the x_proj weights pre-rounded."""
    g = torch.Generator().manual_seed(seed)
    D, N, R = c.D, c.N, c.R
    CD, Lq = R + 2 * N, sc.seq_len(c)
    rq = (lambda t: t.to(HB.t).float()) if mode == "bf16" else (lambda t: t)
    t = dict(xc=rq(torch.randn(B, D, c.H, c.W, generator=g) * 0.5))
    if c.fused:
        t["xw"] = rq(torch.randn(4, CD, D, generator=g) / D ** 0.5)
    else:
        t["xdbl"] = torch.randn(4, B, Lq, CD, generator=g)
    t["dtw"] = (torch.rand(4, D, R, generator=g) * 2 - 1) * R ** -0.5
    t["dtb"] = torch.randn(4, D, generator=g) * 0.5 - 3
    t["A"] = -torch.exp(torch.log(torch.arange(1, N + 1).float())[None].repeat(4 * D, 1) + 0.1 * torch.randn(4 * D, N, generator=g))
    t["Ds"] = 1 + 0.1 * torch.randn(4 * D, generator=g)
    return t


def _run(c, B, mode, t):
    """one call on guarded, NaN-filled buffers -> (y [B,H,W,D] on the GPU, x_dbl [4,B,L,CD] of a fused call or None); the guards and
    the finiteness of the outputs are asserted here"""
    from founddiff_amd import _lib as L
    lib = L.lib()
    D, N, R, H, W = c.D, c.N, c.R, c.H, c.W
    CD, Lq = R + 2 * N, sc.seq_len(c)
    tdt = HB.t if mode == "bf16" else torch.float32
    opts = sc.dtype_opts(c, mode)
    nws = lib.fd_scan_ws_floats(B, H, W, D, N)
    ws = torch.full((nws + GUARD,), float("nan"), device="cuda")
    ws[nws:] = SENTINEL
    ybuf = torch.full((B * H * W + W, D), float("nan"), device="cuda", dtype=tdt)          # + one guard row of the image
    ybuf[B * H * W:] = SENTINEL
    yguard = ybuf[B * H * W:].clone()
    xcd = t["xc"].permute(0, 2, 3, 1).contiguous().to("cuda", tdt)
    d = {k: t[k].contiguous().cuda() for k in ("dtw", "dtb", "A", "Ds")}
    stream = torch.cuda.current_stream().cuda_stream
    if c.fused:
        xwd = t["xw"].to("cuda", tdt).contiguous()
        xdbl = torch.full((4 * B * Lq + 1, CD), float("nan"), device="cuda")
        xdbl[4 * B * Lq:] = SENTINEL
        L.call("fd_selective_scan_xproj", opts, xcd.data_ptr(), xwd.data_ptr(), xdbl.data_ptr(), d["dtw"].data_ptr(), d["dtb"].data_ptr(),
               d["A"].data_ptr(), d["Ds"].data_ptr(), ybuf.data_ptr(), ws.data_ptr(), B, H, W, D, N, R, stream)
    else:
        xdbl = t["xdbl"].contiguous().cuda()
        L.call("fd_selective_scan", opts, xcd.data_ptr(), xdbl.data_ptr(), d["dtw"].data_ptr(), d["dtb"].data_ptr(),
               d["A"].data_ptr(), d["Ds"].data_ptr(), ybuf.data_ptr(), ws.data_ptr(), B, H, W, D, N, R, stream)
    torch.cuda.synchronize()
    y = ybuf[:B * H * W].view(B, H, W, D)
    assert bool(torch.isfinite(y).all()), "y: positions left unwritten (NaN pre-fill) or non-finite"
    assert torch.equal(ybuf[B * H * W:].view(torch.int16 if tdt != torch.float32 else torch.int32),
                       yguard.view(torch.int16 if tdt != torch.float32 else torch.int32)), "the guard row behind y was written"
    assert bool((ws[nws:] == SENTINEL).all()), "the guard behind the workspace was written"
    xd = None
    if c.fused:
        assert bool((xdbl[4 * B * Lq:] == SENTINEL).all()), "the guard row behind x_dbl was written"
        xd = xdbl[:4 * B * Lq].view(4, B, Lq, CD)
        assert bool(torch.isfinite(xd).all()), "x_dbl: rows left unwritten (NaN pre-fill) or non-finite"
    return y, xd


def _params():
    return [pytest.param(c, m, id=f"{case_id(c)}-{m}") for c in SCAN_CASES for m in c.modes]


@pytest.mark.parametrize("c,mode", _params())
def test_scan_form(c, mode):
    from founddiff_amd import _lib as L
    g = geom(L.lib(), c, mode)
    check_expected(c, mode, g)
    t = _inputs(c, c.B, mode)
    ref, xd_rows = scan_reference(t["xc"], t["dtw"], t["dtb"], t["A"], t["Ds"], c.N, c.R, xdbl=t.get("xdbl"), xw=t.get("xw"), f64=True)
    y, xd = _run(c, c.B, mode, t)
    err = rel_err(y.float().cpu().permute(0, 3, 1, 2), ref)
    key = f"scan_forms[{case_id(c)}-{mode}]"
    exd = rel_err(xd.cpu(), xd_rows) if c.fused else None
    print(f"\n{key}: y max-rel {err:.3e}" + (f", x_dbl max-rel {exd:.3e}" if c.fused else "") + f"  geom {g}")
    if c.fused:
        assert exd < (1e-4 if mode == "fp32s" else 1e-5), f"{key}: x_dbl rows {exd:.3e}"
    if mode == "fp32":
        assert err < 1e-5, f"{key}: {err:.3e} >= 1e-5 against the fp64 scan"
    elif mode == "fp32s":
        assert err < 1e-4, f"{key}: {err:.3e} >= 1e-4 against the fp64 scan"
    else:
        gate2x(key, err, 1e-2)


@pytest.mark.parametrize("c,mode", [pytest.param(c, m, id=f"{case_id(c)}-{m}") for c, m in BATCH_CASES])
def test_scan_batch_invariance(c, mode):
    """slice i of a B = 3 call is bitwise the B = 1 call on that slice: the form is a function of the shape, never of the batch"""
    from founddiff_amd import _lib as L
    check_expected(c, mode, geom(L.lib(), c, mode))
    t = _inputs(c, 3, mode, seed=9)
    y3, xd3 = _run(c, 3, mode, t)
    for i in range(3):
        ti = dict(t, xc=t["xc"][i:i + 1])
        if not c.fused:
            ti["xdbl"] = t["xdbl"][:, i:i + 1]
        y1, xd1 = _run(c, 1, mode, ti)
        assert torch.equal(y1[0], y3[i]), f"slice {i}: y differs between B = 1 and B = 3"
        if c.fused:
            assert torch.equal(xd1[:, 0], xd3[:, i]), f"slice {i}: x_dbl differs between B = 1 and B = 3"
