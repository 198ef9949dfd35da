"""Every kernel and tile walk of the fused LayerNorm + modulate -> 1x1 -> depthwise 3x3 family (csrc/fd_pwdw.hip: pwdw_kernel<64>, <128>,
<64, PROJ>, pwdw_gram_kernel, dwconv_gram_kernel; csrc/fd_pwdw32.hip: pwdw32_kernel<DW, 16>, <GRAM, 8>, <PROJ, 8>) against an fp64
restatement.

The cases are tests/pwdw_cases.CASES: every form of fd_pw_dw3x3 the engine can ask for, each entry point at every tiles-per-workgroup
value with an exact and a ragged last workgroup, one tile row / one tile column, operands that are slices of wider rows, zero and
constant rows, sparse images, and 1x1 outputs of a few thousand and of ~1e-5.  tests/test_pwdw_forms_cpu.py asserts that reach without a
GPU, from fd_pw_dw3x3_plan, and checks the bound against an fp32 restatement with seeded faults.

Reference, bound and their derivation: the docstring of tests/pwdw_cases.py.  Comparison: element by element, nothing excluded,
|got - ref| <= bound, for everything the launch stores; the Gram partials per WORKGROUP against the fp64 Gram of that workgroup's own
tiles (fd_pw_dw3x3_plan says which), so that a skipped or doubled tile shows.  On every case the outputs and the partial buffer are
pre-filled with NaN and every owned element comes back finite; slack channels of wider rows, a guard row behind the last pixel and a
guard behind the partials hold a sentinel and come back with their own bits.  After a launch that raised nothing more is launched.

Bit for bit (torch.equal):
  * batch invariance -- image 0 of a B = 4 launch (4 or 8 tiles per workgroup) against the same image alone (1 or 2): "tiles are
    independent: the split does not touch the results" (csrc/fd_pwdw.hip); the Gram kernels: every image of B = 4 against that image
    alone, partials included;
  * across forms -- the v of fd_pw_dw3x3_gram against the v third of fd_pw_dw3x3 at Cdw = 192; the partials without out_v against those
    with it; v under FD_OPT_LOW_LATENCY; fd_pw_dw3x3_proj against the row-GEMM on the stored v, at B = 1 and B = 4;
  * a launch repeated three times.

Largest err / bound per kernel over the table, recorded on an MI355X after the first run (a record of the margin, not a gate; no case
exceeded its bound and no term was added afterwards):
    default build   pwdw_kernel<64> 0.542, <128> 0.425, <64, PROJ> 0.827; pwdw_gram_kernel v 0.352, partials 0.186;
                    dwconv_gram_kernel partials 0.111; pwdw32_kernel<DW, 16> 0.017, <GRAM, 8> partials 0.016, <PROJ, 8> 0.006
    binary16 build  pwdw_kernel<64> 0.633, <128> 0.483, <64, PROJ> 0.932; pwdw_gram_kernel v 0.458, partials 0.179;
                    dwconv_gram_kernel partials 0.113
(PROJ: the output is x + gate . (), and the store rounding of that sum alone reaches 0.9 of its bound.  The Gram partials' bound sums
every pixel's worst case, the errors have random signs: the margin grows with the pixels a workgroup walks -- the sparse cases show
the partials at 0.11 to 0.19.  fp32s: the split and LayerNorm terms are worst cases of errors that mostly cancel.)
The range-lo cases pass with eta = 2^-24: the fp16 tile keeps subnormals, as the comment on dwconv_gram_kernel's halo_store says.
The module takes 9 s on an MI355X (174 tests on both builds, 6 s + 3 s)."""
import ctypes as C
import time

import pytest
import torch

import pwdw_cases as pc
import rows_cases as rc
from conftest import HB, use_half_build
from pwdw_cases import BATCH_CASES, CASES, CROSS_CASES, DW, DWGRAM, F32, GRAM, GRAM32, PROJ, PROJ32, case_id

pytestmark = pytest.mark.gpu

GUARD = 4096                  # floats behind the partial buffer
SENTINEL = -12345.0           # exact in fp32, finite in both 16-bit types: slack and guards are compared with their own bits
DEV = "cuda"
_T0 = []


@pytest.fixture(scope="module", params=["bf16-build", "fp16-build"], autouse=True)
def half_build(request):
    """every test of this module once per build of the library (conftest.use_half_build)"""
    use_half_build(request.param == "fp16-build")
    _CACHE.clear()
    _T0.append(time.time())
    yield request.param
    use_half_build(False)
    _CACHE.clear()
    if _MAXR:
        print(f"\npwdw_forms[{request.param}]: largest err / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(_MAXR.items()))
              + f"; {time.time() - _T0.pop():.0f} s")
    _MAXR.clear()


@pytest.fixture(autouse=True)
def _default_build_only(request, half_build):
    """the fp32-storage kernels belong to the default build: not repeated on the binary16 one"""
    if half_build == "fp16-build":
        c = getattr(request.node, "callspec", None) and request.node.callspec.params.get("c")
        if c is not None and pc.is32(c):
            pytest.skip("default build only")


_CACHE = {}       # the operands (CPU and device) of the case that ran last
_MAXR = {}        # kernel -> largest err / bound seen (a record, not a gate)
_FAULTED = []     # the launch that raised, if one did: the device may be in no state to go on


def _tdt(c):
    return torch.float32 if pc.is32(c) else HB.t


def _rq(c):
    return (lambda v: v) if pc.is32(c) else (lambda v: v.to(HB.t).float())


def _to_device(c, t):
    from founddiff_amd.engine import DAEngine
    d = {}
    for k, v in t.items():
        if k in ("x", "qkv") or (k in ("w_pw", "w2") and not pc.is32(c)):
            d[k] = v.to(DEV, _tdt(c)).contiguous()
        elif k in ("w_hi", "w_lo"):
            d[k] = v.to(DEV, torch.bfloat16).contiguous()
        elif k == "taps" and not pc.is32(c):
            d[k] = DAEngine._dw_masked(v.to(DEV))                  # fp16 channel pairs: the values are fp16 already, the cast is exact
        else:
            d[k] = v.to(DEV, torch.float32).contiguous()
    return d


def _operands(c, seed=11):
    key = (case_id(c), c.B, _tdt(c), seed)
    if _CACHE.get("key") != key:
        _CACHE.clear()
        t = pc.make_inputs(c, _rq(c), seed)
        _CACHE.update(key=key, t=t, d=_to_device(c, t))
    return _CACHE["t"], _CACHE["d"]


def _bits(x):
    return x.view(torch.int32 if x.dtype == torch.float32 else torch.int16)


class _Out:
    """a guarded output [B H W + 1 rows][ld] of which channels [off, off + n) are owned: NaN there, the sentinel elsewhere"""

    def __init__(self, c, ld, off, n, dt):
        self.rows, self.ld, self.off, self.n, self.shape = c.B * pc.npx(c), ld, off, n, (c.B, c.H, c.W, n)
        self.buf = torch.full((self.rows + 1, ld), float("nan"), device=DEV, dtype=dt)
        self.buf[:, :off] = SENTINEL
        self.buf[:, off + n:] = SENTINEL
        self.buf[self.rows:] = SENTINEL
        self.before = self.buf.clone()

    def ptr(self):
        return self.buf.data_ptr()

    def take(self, what):
        own = self.buf[:self.rows, self.off:self.off + self.n]
        assert bool(torch.isfinite(own).all()), f"{what}: elements left unwritten (NaN pre-fill) or non-finite"
        got = own.reshape(self.shape).clone()
        self.buf[:self.rows, self.off:self.off + self.n] = 0
        self.before[:self.rows, self.off:self.off + self.n] = 0
        assert torch.equal(_bits(self.buf), _bits(self.before)), f"{what}: slack channels or the guard row behind the output were written"
        return got


def _run(c, d):
    """one launch on guarded, NaN-filled buffers -> {output name: tensor as stored} and the plan under "plan" """
    from founddiff_amd import _lib as L
    if _FAULTED:
        pytest.fail(f"the launch of {_FAULTED[0]} raised: nothing more is launched from this module")
    lib, ge, dt = L.lib(), pc.geom(c), _tdt(c)
    pl = pc.plan(lib, c)
    assert pl is not None, f"{case_id(c)}: refused by {c.entry}"
    P = lambda k, off=0: d[k].data_ptr() + 4 * off                         # (fp32 operands)
    outs, part = {}, None
    heads = pc.gram_slices(c)[2] if c.entry in (GRAM, DWGRAM, GRAM32) else 0
    if heads:
        n = c.B * heads * pl["gx"] * 1088
        part = torch.full((n + GUARD,), float("nan"), device=DEV)
        part[n:] = SENTINEL
    opts = pc.dtype_opts(c)
    ln = lambda: (P("ln_gamma") if c.affine else None, P("ln_beta") if c.affine else None, pc.EPS, P("ln_mod", ge.shift_off),
                  P("ln_mod", ge.scale_off), ge.ln_ld)
    xa = lambda: (d["x"].data_ptr(), ge.ld_x, ge.off_x, c.cin)
    gate = lambda: (P("ln_mod", ge.gate_off) if c.strided else P("gate"), ge.gate_ld)
    bias = d["b_dw"].data_ptr() if c.bias else None
    tail = (c.B, c.H, c.W, torch.cuda.current_stream().cuda_stream)
    if c.entry in (DW, F32):
        outs["out_dw"] = _Out(c, ge.ld_dw, ge.off_dw, c.cdw, dt)
    if c.entry == DW and c.cz:
        outs["z"] = _Out(c, ge.ld_z, ge.off_z, c.cz, dt)
    if c.entry in (PROJ, PROJ32):
        outs["out"] = _Out(c, ge.ld_dw, ge.off_dw, 64, dt)
    if c.entry == GRAM and c.out_v:
        outs["v"] = _Out(c, ge.ld_dw, ge.off_dw, 64, dt)
    if c.entry == DW:
        z = outs.get("z")
        args = (opts, *xa(), *ln(), d["w_pw"].data_ptr(), c.cdw, d["taps"].data_ptr(), bias, int(c.silu), outs["out_dw"].ptr(), ge.ld_dw,
                ge.off_dw, c.cz, z.ptr() if z else None, ge.ld_z if z else 0, ge.off_z if z else 0, *tail)
    elif c.entry == PROJ:
        args = (opts, *xa(), *ln(), d["w_pw"].data_ptr(), d["taps"].data_ptr(), d["w2"].data_ptr(), *gate(), outs["out"].ptr(), ge.ld_dw,
                ge.off_dw, *tail)
    elif c.entry == GRAM:
        v = outs.get("v")
        args = (opts, *xa(), *ln(), d["w_pw"].data_ptr(), d["taps"].data_ptr(), v.ptr() if v else None, ge.ld_dw if v else 0,
                ge.off_dw if v else 0, part.data_ptr(), *tail)
    elif c.entry == DWGRAM:
        args = (opts, d["qkv"].data_ptr(), ge.ld_qkv, c.C, d["taps"].data_ptr(), part.data_ptr(), *tail)
    elif c.entry == F32:
        args = (*xa(), *ln(), d["w_hi"].data_ptr(), d["w_lo"].data_ptr(), c.cdw, d["taps"].data_ptr(), bias, int(c.silu),
                outs["out_dw"].ptr(), ge.ld_dw, ge.off_dw, *tail)
    elif c.entry == GRAM32:
        args = (*xa(), *ln(), d["w_hi"].data_ptr(), d["w_lo"].data_ptr(), d["taps"].data_ptr(), ge.ld_wdw, part.data_ptr(), *tail)
    else:
        args = (*xa(), *ln(), d["w_hi"].data_ptr(), d["w_lo"].data_ptr(), d["taps"].data_ptr(), ge.ld_wdw, d["w2"].data_ptr(), *gate(),
                outs["out"].ptr(), ge.ld_dw, ge.off_dw, *tail)
    try:
        L.call(c.entry, *args)
        torch.cuda.synchronize()
    except Exception:
        _FAULTED.append(case_id(c))
        raise
    r = {k: o.take(f"{case_id(c)}: {k}") for k, o in outs.items()}
    if heads:
        n = part.numel() - GUARD
        assert bool((part[n:] == SENTINEL).all()), f"{case_id(c)}: the guard behind the partials was written"
        assert bool(torch.isfinite(part[:n]).all()), f"{case_id(c)}: partials left unwritten (NaN pre-fill) or non-finite"
        r["part"] = part[:n].view(c.B, heads, pl["gx"], 1088).clone()
    r["plan"] = pl
    return r


def _where(c, k, idx, pl):
    if k == "part":
        b, h, g, e = idx
        what = f"Gram row {e // 32}, column {e % 32}" if e < 1024 else ("sum q^2" if e < 1056 else "sum k^2") + f" of channel {e % 32}"
        return f"(image {b}, head {h}, workgroup {g} = tiles {g * pl['tpw']} .. {min(pl['ntiles'], (g + 1) * pl['tpw']) - 1}): {what}"
    return f"(image, y, x, channel) {idx}: {pc.where_in_tile(idx, pl['TW'])}"


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_pwdw_form(c):
    t, d = _operands(c)
    got = _run(c, d)
    pl = got["plan"]
    ref = pc.pwdw_reference(c, t, _tdt(c), DEV)
    eb = pc.error_bounds(c, t, ref, _tdt(c), pl, DEV)
    assert set(eb) == set(got) - {"plan"}, (sorted(eb), sorted(got))
    msgs, bad = [], False
    for k, (rf, bound) in eb.items():
        r, idx, e, b = pc.worst((got[k].double() - rf).abs(), bound)
        msgs.append(f"{k}: max err / bound {r:.3f} at {_where(c, k, idx, pl)}: |got - ref| = {e:.3e}, bound {b:.3e}")
        _MAXR[pl["kernel"] + (" part" if k == "part" else "")] = max(_MAXR.get(pl["kernel"] + (" part" if k == "part" else ""), 0.0), r)
        bad |= not r <= 1.0
    msg = f"pwdw_forms[{case_id(c)}] {pl['kernel']}, {pl['tpw']} tiles per workgroup: " + "; ".join(msgs)
    print("\n" + msg)
    assert not bad, msg


def _same(a, b, what, keys=None):
    for k in keys or [k for k in a if k != "plan"]:
        same = _bits(a[k]) == _bits(b[k])
        assert bool(same.all()), (f"{what}: {int((~same).sum())} of {same.numel()} elements of {k} differ, first at "
                                  f"{tuple(int(v) for v in (~same).nonzero()[0])}")


@pytest.mark.parametrize("c", [c for c in CASES if c.name in pc.REPEAT], ids=case_id)
def test_repeat_launches(c):
    """a launch repeated on fresh buffers reproduces the first result bit for bit"""
    _, d = _operands(c)
    first = _run(c, d)
    for i in range(3):
        _same(first, _run(c, d), f"repeat {i + 1}")


@pytest.mark.parametrize("c", BATCH_CASES, ids=case_id)
def test_batch_invariance(c):
    """image 0 of the B = 4 launch (4 or 8 tiles per workgroup) and the same image alone (1 or 2): the same bits.  The Gram kernels walk
    the same tiles per workgroup at any batch: every image of B = 4 against that image alone, partials included"""
    t, d = _operands(c, seed=17)
    out4 = _run(c, d)
    gram = c.entry in (GRAM, DWGRAM, GRAM32)
    for i in range(4 if gram else 1):
        c1, t1 = pc.batch_slice(c, t, i)
        out1 = _run(c1, _to_device(c1, t1))
        assert out1["plan"]["kernel"] == out4["plan"]["kernel"]
        assert gram or out1["plan"]["tpw"] * 4 == out4["plan"]["tpw"], (out1["plan"], out4["plan"])
        for k in out1:
            if k != "plan":
                same = _bits(out1[k][0]) == _bits(out4[k][i])
                assert bool(same.all()), (f"{k}: {int((~same).sum())} of {same.numel()} elements of image {i} differ between B = 1 and "
                                          f"B = 4, first at {tuple(int(v) for v in (~same).nonzero()[0])}")


@pytest.mark.parametrize("c", CROSS_CASES, ids=case_id)
def test_across_forms(c):
    """one qkv block four ways: fd_pw_dw3x3_gram with and without out_v, under FD_OPT_LOW_LATENCY, fd_pw_dw3x3 at Cdw = 192, and the v
    branch through fd_pw_dw3x3_proj against the row-GEMM on the stored v"""
    from founddiff_amd import _lib as L
    t, d = _operands(c, seed=19)
    g = _run(c, d)
    _same(g, _run(c._replace(out_v=False), d), "partials without out_v", keys=["part"])
    ll = _run(c._replace(lowlat=True), d)
    assert ll["plan"]["tpw"] == 4 and g["plan"]["tpw"] == 8
    _same(g, ll, "v under FD_OPT_LOW_LATENCY", keys=["v"])
    cd = pc._p(c.name + "-dw192", DW, c.B, (c.H, c.W), cdw=192, affine=False, bias=False, silu=False)
    full = _run(cd, d)["out_dw"]
    same = _bits(full[..., 128:]) == _bits(g["v"])
    assert bool(same.all()), f"{int((~same).sum())} elements of v differ between fd_pw_dw3x3_gram and fd_pw_dw3x3 at Cdw = 192"
    # the v branch: LN -> W_v -> depthwise -> Weff[b] -> x + gate . (), against the row-GEMM on the STORED v
    cp = pc._p(c.name + "-proj", PROJ, c.B, (c.H, c.W), affine=False)
    gen = torch.Generator().manual_seed(23)
    w2 = (torch.randn(c.B, 64, 64, generator=gen) / 8).to(DEV, HB.t)
    gate = (0.5 * torch.randn(c.B, 64, generator=gen)).to(DEV)
    wv = d["w_pw"][128:].contiguous()
    taps_v = d["taps"][:, 64:].contiguous()                               # [9][96 words] -> the 32 words of the v channels
    fused = _run(cp, dict(d, w_pw=wv, taps=taps_v, w2=w2, gate=gate))["out"]
    rcase = rc._r("v-branch", c.B, (c.H, c.W), 64, 64, bias=False, wb=True, epi="GATE_RES", modes=("bf16",))
    out = torch.full((c.B, c.H, c.W, 64), float("nan"), device=DEV, dtype=HB.t)
    ptrs = dict(rc.DUMMY_PTRS, in0=g["v"].data_ptr(), weight=w2.data_ptr(), res=d["x"].data_ptr(), gate=gate.data_ptr(), out=out.data_ptr())
    p = rc.params_for(rcase, "bf16", ptrs)
    assert L.rows_form(L.lib(), p) is not None
    L.call("fd_conv2d", C.byref(p), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    same = _bits(fused) == _bits(out)
    assert bool(same.all()), f"{int((~same).sum())} of {same.numel()} elements differ between fd_pw_dw3x3_proj and the row-GEMM on the stored v"
