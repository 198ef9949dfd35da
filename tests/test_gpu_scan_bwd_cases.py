"""Every instantiation and tiling edge of the two scan backwards against float64.

The cases are tests/scan_bwd_cases.CS_CASES (fd_cross_scan_fwd_f32 + fd_cross_scan_bwd_f32 and their NHWC twins) and SB_CASES
(fd_selective_scan_bwd_f32); tests/test_scan_bwd_cases_cpu.py asserts, without a GPU, that they reach all 20 (N, R) instantiations
in both layouts, both tile lengths, last tiles / lanes / x_proj blocks of every awkward length, H = 1 and W = 1, every channel
split and both sides of its threshold; every state-chunk and row-split form of the reference layout; and both branches of
softplus' derivative.  The references are scan_bwd_ref.scan_grads_f64 and the float64 composition scan_bwd_cases.cs_reference, run
on the GPU.

The calls go through the C ABI, so the test owns every buffer: every output is pre-filled with NaN and followed by a 64-float guard
in the same allocation, the workspaces are exactly *_ws_floats long, NaN-filled and guarded too.  After a call every output is
finite and every guard has its bits; a second call gives the same bits everywhere.

Gates (rel_err = max abs error over the reference's max abs): 1e-5 for y, x_dbl and the per-position gradients -- the project's
fp32-against-fp64 gate (test_gpu_scan_forms.py) -- and 1e-4 for the gradients summed over batch x L; and 4 x the error recorded
on an MI355X in tests/golden/scan_bwd_measured_errors.json, floor 1e-6 (scan_bwd_cases.gate4x).  The table's second column is the
error of the same restatement run in float32: the kernels' errors lie within a small factor of it."""
import time

import pytest
import torch

import scan_bwd_cases as sc
from conftest import rel_err
from scan_bwd_cases import CS_BATCH_IDS, CS_CASES, LAYOUTS, SB_CASES, check_expected, cs_geom, cs_id, gate4x, sb_geom, sb_id
from scan_bwd_ref import scan_grads_f64

pytestmark = pytest.mark.gpu

GUARD = 64                    # floats behind every output and workspace
SENTINEL = -12345.0


class _Buf:
    """n floats of NaN and a guard behind them, in one allocation"""

    def __init__(self, *shape):
        self.n = 1
        for s in shape:
            self.n *= s
        self.all = torch.full((self.n + GUARD,), float("nan"), device="cuda")
        self.all[self.n:] = SENTINEL
        self.t = self.all[:self.n].view(*shape)

    def ptr(self):
        return self.all.data_ptr()

    def check(self, name, finite=True):
        want = torch.full((GUARD,), SENTINEL, device="cuda").view(torch.int32)
        assert torch.equal(self.all[self.n:].view(torch.int32), want), f"the guard behind {name} was written"
        if finite:
            assert bool(torch.isfinite(self.t).all()), f"{name}: elements left unwritten (NaN pre-fill) or non-finite"


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---- the cross-scan --------------------------------------------------------------------------------------------------------------
def _cs_run(c, B, layout, x, dy, p):
    """forward + backward of one layout on guarded buffers -> {name: tensor} as sc.CS_OUTPUTS names them (dx in the layout's own
    order); the guards and the finiteness of the outputs are asserted here"""
    from founddiff_amd import _lib as L
    lib = L.lib()
    D, N, R, H, W = c.D, c.N, c.R, c.H, c.W
    CD, Lq = R + 2 * N, ((H + 1) // 2) * ((W + 1) // 2)
    d = {k: p[k].contiguous().cuda() for k in ("x_proj_weight", "dt_projs_weight", "dt_projs_bias", "A", "Ds")}
    pw = [d[k].data_ptr() for k in ("x_proj_weight", "dt_projs_weight", "dt_projs_bias", "A", "Ds")]
    dyd = dy.contiguous().cuda()
    nhwc = layout == "nhwc"
    o = dict(x_dbl=_Buf(4, B, Lq, CD), y=_Buf(B, H, W, D), dx=_Buf(B, H, W, D) if nhwc else _Buf(B, D, H, W),
             dx_proj_w=_Buf(4, CD, D), ddtw=_Buf(4, D, R), ddtb=_Buf(4, D), dA=_Buf(4 * D, N), dDs=_Buf(4 * D))
    wf = _Buf(lib.fd_scan_ws_floats(B, H, W, D, N))
    nws = lib.fd_cross_scan_bwd_ws_floats(B, H, W, D, N, R)
    assert nws > 0
    wb = _Buf(nws)
    dims = (B, H, W, D, N, R, _stream())
    if nhwc:
        xc = x.permute(0, 2, 3, 1).contiguous().cuda()
        L.call("fd_cross_scan_fwd_nhwc_f32", xc.data_ptr(), *pw, o["x_dbl"].ptr(), o["y"].ptr(), wf.ptr(), *dims)
        xcp = xc.data_ptr()
    else:
        xd = x.contiguous().cuda()
        o["xc"] = _Buf(B, H, W, D)
        L.call("fd_cross_scan_fwd_f32", xd.data_ptr(), *pw, o["xc"].ptr(), o["x_dbl"].ptr(), o["y"].ptr(), wf.ptr(), *dims)
        xcp = o["xc"].ptr()
    L.call("fd_cross_scan_bwd_nhwc_f32" if nhwc else "fd_cross_scan_bwd_f32", xcp, o["x_dbl"].ptr(), *pw, dyd.data_ptr(),
           o["dx"].ptr(), o["dx_proj_w"].ptr(), o["ddtw"].ptr(), o["ddtb"].ptr(), o["dA"].ptr(), o["dDs"].ptr(), wb.ptr(), *dims)
    torch.cuda.synchronize()
    for name, b in o.items():
        b.check(f"{name} ({layout})")
    wf.check("the forward's workspace", finite=False)
    wb.check("the backward's workspace", finite=False)
    if not nhwc:
        assert torch.equal(o["xc"].t, x.permute(0, 2, 3, 1).contiguous().cuda()), "xc is not x in NHWC"
    return {k: b.t for k, b in o.items() if k != "xc"}


_cs_cache = {}


def _cs_ref(c):
    """(inputs, float64 reference, float32 restatement's errors) of a case, computed once for its two layouts"""
    key = cs_id(c)
    if key not in _cs_cache:
        _cs_cache.clear()
        x, dy, p = sc.cs_inputs(c)
        ref = sc.cs_reference(x, dy, p, "cuda", torch.float64)
        f32 = sc.cs_reference(x, dy, p, "cuda", torch.float32)
        _cs_cache[key] = (x, dy, p, ref, {k: rel_err(f32[k], ref[k]) for k in sc.CS_OUTPUTS})
    return _cs_cache[key]


@pytest.mark.parametrize("c,layout", [pytest.param(c, lay, id=f"{cs_id(c)}-{lay}") for c in CS_CASES for lay in LAYOUTS])
def test_cross_scan_case(c, layout):
    from founddiff_amd import _lib as L
    t0 = time.time()
    g = cs_geom(L.lib(), c)
    check_expected(cs_id(c), c.expect, g)
    x, dy, p, ref, ef32 = _cs_ref(c)
    got = _cs_run(c, c.B, layout, x, dy, p)
    again = _cs_run(c, c.B, layout, x, dy, p)
    for name in sc.CS_OUTPUTS:
        assert torch.equal(got[name], again[name]), f"{name}: a second call gives other bits"
    errs = {}
    for name in sc.CS_OUTPUTS:
        r = ref[name].permute(0, 2, 3, 1) if (name == "dx" and layout == "nhwc") else ref[name]
        assert got[name].shape == r.shape, (name, got[name].shape, r.shape)
        errs[name] = rel_err(got[name], r)
    torch.cuda.synchronize()
    print(f"\ncs[{cs_id(c)}-{layout}] {time.time() - t0:.2f} s  geom {g}")
    for name in sc.CS_OUTPUTS:
        print(f"  {name:10s} kernel {errs[name]:.3e}   float32 restatement {ef32[name]:.3e}")
    for name in sc.CS_OUTPUTS:
        gate4x(f"cs[{cs_id(c)}-{layout}].{name}", errs[name], ef32[name],
               sc.POSITION_GATE if name in sc.CS_POSITION else sc.SUMMED_GATE)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("cid", CS_BATCH_IDS)
def test_cross_scan_batch_invariance(cid, layout):
    """slice i of a B = 3 call is bitwise the B = 1 call on that slice, y and dx: tile length, channel split and every reduction
    order are functions of (H, W, D, N, R) only"""
    c = {cs_id(k): k for k in CS_CASES}[cid]
    x, dy, p = sc.cs_inputs(c, B=3, seed=9)
    g3 = _cs_run(c, 3, layout, x, dy, p)
    for i in range(3):
        g1 = _cs_run(c, 1, layout, x[i:i + 1], dy[i:i + 1], p)
        assert torch.equal(g1["y"][0], g3["y"][i]), f"slice {i}: y differs between B = 1 and B = 3"
        assert torch.equal(g1["dx"][0], g3["dx"][i]), f"slice {i}: dx differs between B = 1 and B = 3"


# ---- the reference layout --------------------------------------------------------------------------------------------------------
def _sb_run(c, ins):
    """one call on guarded buffers -> the seven outputs (None where the case has no D / delta_bias)"""
    from founddiff_amd import _lib as L
    lib = L.lib()
    u, delta, A, Bm, Cm, D, bias, dout = ins
    b, KD, K, N, Ln = c.batch, c.KD, c.K, c.N, c.L
    bc = (b, N, Ln) if K == 1 else (b, K, N, Ln)                      # a single group: B / C are 3-D, as the reference passes them
    o = dict(du=_Buf(b, KD, Ln), ddelta=_Buf(b, KD, Ln), dA=_Buf(KD, N), dB=_Buf(*bc), dC=_Buf(*bc),
             dD=_Buf(KD) if D is not None else None, ddelta_bias=_Buf(KD) if bias is not None else None)
    nws = lib.fd_selective_scan_bwd_ws_floats(b, KD, K, N, Ln)
    assert nws > 0
    ws = _Buf(nws)
    p = lambda t: None if t is None else t.data_ptr()
    q = lambda k: None if o[k] is None else o[k].ptr()
    L.call("fd_selective_scan_bwd_f32", p(u), p(delta), p(A), p(Bm), p(Cm), p(D), p(bias), p(dout), int(c.softplus), c.nrows,
           b, KD, K, N, Ln, q("du"), q("ddelta"), q("dA"), q("dB"), q("dC"), q("dD"), q("ddelta_bias"), ws.ptr(), _stream())
    torch.cuda.synchronize()
    for name, buf in o.items():
        if buf is not None:
            buf.check(name)
    ws.check("the workspace", finite=False)
    return {k: (None if buf is None else buf.t) for k, buf in o.items()}


@pytest.mark.parametrize("c", [pytest.param(c, id=sb_id(c)) for c in SB_CASES])
def test_reference_layout_case(c):
    from founddiff_amd import _lib as L
    t0 = time.time()
    g = sb_geom(L.lib(), c)
    check_expected(sb_id(c), c.expect, g)
    ins = [None if t is None else t.cuda() for t in sc.sb_inputs(c)]
    if c.K == 1:
        ins[3], ins[4] = ins[3][:, 0], ins[4][:, 0]
    got = _sb_run(c, ins)
    again = _sb_run(c, ins)
    ref_ins = list(ins)
    if c.K == 1:
        ref_ins[3], ref_ins[4] = ins[3].unsqueeze(1), ins[4].unsqueeze(1)
    ref = dict(zip(sc.SB_OUTPUTS, scan_grads_f64(*ref_ins, c.softplus)))
    f32 = dict(zip(sc.SB_OUTPUTS, scan_grads_f64(*ref_ins, c.softplus, dtype=torch.float32)))
    errs, ef32 = {}, {}
    for name in sc.SB_OUTPUTS:
        if ref[name] is None:
            assert got[name] is None and name in ("dD", "ddelta_bias"), name
            continue
        assert torch.equal(got[name], again[name]), f"{name}: a second call gives other bits"
        r = ref[name][:, 0] if (c.K == 1 and name in ("dB", "dC")) else ref[name]
        f = f32[name][:, 0] if (c.K == 1 and name in ("dB", "dC")) else f32[name]
        assert got[name].shape == r.shape, (name, got[name].shape, r.shape)
        errs[name], ef32[name] = rel_err(got[name], r), rel_err(f, r)
    torch.cuda.synchronize()
    print(f"\nsb[{sb_id(c)}] {time.time() - t0:.2f} s  geom {g}")
    for name in errs:
        print(f"  {name:12s} kernel {errs[name]:.3e}   float32 restatement {ef32[name]:.3e}")
    for name in errs:
        gate4x(f"sb[{sb_id(c)}].{name}", errs[name], ef32[name], sc.POSITION_GATE if name in sc.SB_POSITION else sc.SUMMED_GATE)
