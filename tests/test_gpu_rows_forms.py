"""Every instantiation and tile walk of the streaming row-GEMM (fd_conv_kernel_id 10: csrc/fd_gemm_rows.hip, 16-bit storage; 17:
csrc/fd_gemm_rows32.hip, fp32 storage with split-bf16 contractions) against an fp64 restatement.

The cases are tests/rows_cases.rows_cases(): one per compiled form the dispatcher can reach (169 of gemm_rows_kernel, 120 of
gemm_rows32_kernel), the three reachable z-recompute kernels, the edges of the pixel, channel and K axes, of the operand strides and of
the fused LayerNorm prologues, and the persistent tile walk with one and with several tiles per wave.  tests/test_rows_forms_cpu.py
asserts that reach without a GPU, from fd_gemm_rows_form.  gemm_rows_zre_kernel<4, 256, false> runs only under a development switch
that the tested build compiles away: out of scope.

Reference (rows_cases.rows_reference, fp64 on the device, from the operands' stored values): the prologue -- LayerNorm with the biased
variance, then modulate or gate; for the z-recompute kernels z = SiLU(W_z . LNmod(res)) -- F.linear, bias and epilogue, and for
GNSILU_ADD_FINAL the dot with fin_w, fin_b and the fin_mode update of fin_img.

Comparison: element by element, nothing excluded, |got - ref| <= bound with (rows_cases.error_bounds)
    bound = u_out |ref| + L (c_mode S + S_pro) + 2^-20 (|ref| + |addend|)
u_out, L, c_mode = (K + 8) 2^-24 (+ 2^-14 split), S = sum |w| |a| + |bias| and the last term as conv_cases.error_bounds;
    S_pro = sum_k |w_nk| (u_op |a_k| + c_ln abar_k)
for a fused prologue: a its fp64 output, abar the same with every term replaced by its magnitude (G and Bc term by term, see
rows_cases.prologue), u_op the unit roundoff of the 16-bit type the prologue result is packed to (0 in fp32s).  c_ln = 4 x 2.03e-6: the
figure is measured with fp32 torch against the fp64 reference on the table's own inputs (rows_cases.C_LN_MEASURED), never against the
kernel.  Z-recompute: the operand's error gains |LN(y)| dz, dz = u_h |z| + 1.1 (c_mode S_z + S_pro,z) -- an absolute error of z, so it
enters S_pro beside c_ln abar, not under c_ln.  GNSILU_ADD_FINAL: fin_out within sum |fin_w_n| bound_n + (Cout + 4) 2^-24
sum |fin_w_n ref_n|; fin_img within |fin_alpha| (1 in the last step) times that + 2^-23 (|fin_img| + |x_in| + 1) for the update's own
two fp32 operations.
Largest err / bound over the table, recorded on an MI355X (a record of the margin, not a gate):
    default build   bf16: plain 0.996, prologue 0.981, z-recompute 0.910, final 0.450
                    fp32s: plain 0.129, prologue 0.154, z-recompute 0.014, final 0.013
    binary16 build  plain 0.994, prologue 0.986, z-recompute 0.933, final 0.461
(In the 16-bit modes the store rounding alone reaches 0.99 of the bound at elements just above a power of two -- u_out is exactly that
rounding; the fp32s rows show the margin of the contraction and of the prologue.  The z-recompute bound is the widest: dz sums the
roundings of W_z's 64 or 128 packed operands linearly.)  No case exceeded the bound and no term had to be added after the first run;
the module takes 22 s on an MI355X (633 launches' tests on both builds).

On every case the output is pre-filled with NaN and every owned element comes back finite; slack channels of wider rows, a guard row
behind the last pixel and guards behind fin_out / fin_img hold a sentinel and come back with their own bits; under GNSILU_ADD_FINAL
p.out comes back entirely untouched (the kernel stores nothing there).  After a launch that raised nothing more is launched.

Bit for bit (torch.equal), on a handful of cases per family:
  * batch invariance -- image 0 of a B = 4 launch against the same image alone (B = 1 moves the workgroups-per-CU limit from 3 to 4,
    the grid, and the walk from several tiles per wave to one): "The grid size does not touch the results: every pixel row is computed
    by itself" (csrc/fd_gemm_rows.hip);
  * column invariance -- the first 64 output channels of an NT 512 and an NT 768 launch against a Cout = 64 launch (NT 256) on the same
    leading weight rows; the fp32s whole launch against DAEngine.conv_cols chunks, which relies on it;
  * a launch repeated three times."""
import ctypes as C

import pytest
import torch

import rows_cases as rc
from conftest import HB, use_half_build
from rows_cases import BATCH_CASES, COLUMN_CASES, case_id

pytestmark = pytest.mark.gpu

GUARD = 64                    # floats behind fin_out / fin_img
SENTINEL = -12345.0           # exact in fp32, finite in both 16-bit types: slack and guards are compared with their own bits
DEV = "cuda"


@pytest.fixture(scope="module", params=["bf16-build", "fp16-build"], autouse=True)
def half_build(request):
    """every test of this module once per build of the library (conftest.use_half_build)"""
    use_half_build(request.param == "fp16-build")
    _CACHE.clear()
    yield request.param
    use_half_build(False)
    _CACHE.clear()
    if _MAXR:
        print(f"\nrows_forms[{request.param}]: largest err / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(_MAXR.items())))
    _MAXR.clear()


@pytest.fixture(autouse=True)
def _default_build_only(request, half_build):
    """the fp32-storage mode belongs to the default build: not repeated on the binary16 one"""
    if half_build == "fp16-build":
        mode = getattr(request.node, "callspec", None) and request.node.callspec.params.get("mode")
        if mode == "fp32s":
            pytest.skip("default build only")


_CACHE = {}       # the operands (CPU and device) and the reference of the case that ran last
_MAXR = {}        # "mode what" -> largest err / bound seen (a record, not a gate)
_FAULTED = []     # the launch that raised, if one did: the device may be in no state to go on

_STORED = ("in0", "in1", "weight", "res", "h", "z", "zre_w")      # operands in the storage type; everything else is fp32


def _tdt(mode):
    return HB.t if mode == "bf16" else torch.float32


def _operands(c, mode, seed=11):
    """(operands on the CPU in fp32, the same on the device in their stored types)"""
    key = (case_id(c), c.B, c.cout, _tdt(mode), seed)
    if _CACHE.get("key") != key:
        rq = (lambda t: t.to(HB.t).float()) if mode == "bf16" else (lambda t: t)
        _CACHE.clear()
        t = rc.make_inputs(c, rq, seed)
        _CACHE.update(key=key, t=t, d=_to_device(t, mode))
    return _CACHE["t"], _CACHE["d"]


def _to_device(t, mode):
    return {k: v.to(DEV, _tdt(mode) if k in _STORED else torch.float32).contiguous() for k, v in t.items()}


def _reference(c, mode):
    t, _ = _operands(c, mode)
    if "ref" not in _CACHE:
        _CACHE["ref"] = rc.rows_reference(c, t, mode, _tdt(mode), DEV)
    return _CACHE["ref"]


def _bits(x):
    return x.view(torch.int32 if x.dtype == torch.float32 else torch.int16)


def _run(c, mode, d, expect=None):
    """one fd_conv2d launch on guarded, NaN-filled buffers -> dict: out [B, P, Cout] in its stored type (None under GNSILU_ADD_FINAL),
    fin_out / fin_img [B, P] fp32; the plan, the guards and the finiteness of what was written are asserted here"""
    from founddiff_amd import _lib as L
    if _FAULTED:
        pytest.fail(f"the launch of {_FAULTED[0]} raised: nothing more is launched from this module")
    lib = L.lib()
    tdt, P, rows = _tdt(mode), rc.npx(c), c.B * rc.npx(c)
    final = c.epi == "GNSILU_ADD_FINAL"
    buf = torch.full((rows + 1, c.ldo), float("nan"), device=DEV, dtype=tdt)            # + a guard row
    buf[:, :c.offo] = SENTINEL
    buf[:, c.offo + c.cout:] = SENTINEL
    buf[rows:] = SENTINEL
    before = buf.clone()
    ptrs = {k: v.data_ptr() for k, v in d.items()}
    ptrs["out"] = buf.data_ptr()
    fo = fi = None
    if final:
        fo = torch.full((rows + GUARD,), float("nan"), device=DEV)
        fo[rows:] = SENTINEL
        ptrs["fin_out"] = fo.data_ptr()
        if c.fin_mode:
            fi = torch.full((rows + GUARD,), SENTINEL, device=DEV)
            fi[:rows] = d["fin_img"].flatten()
            ptrs["fin_img"] = fi.data_ptr()
    p = rc.params_for(c, mode, ptrs)
    f = L.rows_form(lib, p)
    assert f is not None and f["kid"] == rc.KID[mode] == lib.fd_conv_kernel_id(C.byref(p)), f"{case_id(c)}-{mode}: not on the row-GEMM: {f}"
    if expect is not None:
        assert {k: f[k] for k in expect} == expect, f"{case_id(c)}-{mode}: plan {f}, expected {expect}"
    try:
        L.call("fd_conv2d", C.byref(p), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    except Exception:
        _FAULTED.append(f"{case_id(c)}-{mode}")
        raise
    r = dict(out=None, fin_out=None, fin_img=None, form=f)
    if final:
        assert torch.equal(_bits(buf), _bits(before)), "GNSILU_ADD_FINAL wrote through p.out"
        assert bool((fo[rows:] == SENTINEL).all()), "the guard behind fin_out was written"
        r["fin_out"] = fo[:rows].view(c.B, P).clone()
        assert bool(torch.isfinite(r["fin_out"]).all()), "fin_out: elements left unwritten (NaN pre-fill) or non-finite"
        if c.fin_mode:
            assert bool((fi[rows:] == SENTINEL).all()), "the guard behind fin_img was written"
            r["fin_img"] = fi[:rows].view(c.B, P).clone()
            assert bool(torch.isfinite(r["fin_img"]).all()), "fin_img: non-finite"
        return r
    own = buf[:rows, c.offo:c.offo + c.cout]
    assert bool(torch.isfinite(own).all()), "out: elements left unwritten (NaN pre-fill) or non-finite"
    r["out"] = own.reshape(c.B, P, c.cout).clone()
    buf[:rows, c.offo:c.offo + c.cout] = 0
    before[:rows, c.offo:c.offo + c.cout] = 0
    assert torch.equal(_bits(buf), _bits(before)), "slack channels or the guard row behind the output were written"
    return r


def _worst(err, bound):
    """largest err / bound and where; a bound of exactly 0 admits err = 0 only"""
    bound = bound.expand_as(err)
    ratio = torch.where(bound > 0, err / bound, torch.where(err > 0, float("inf"), 0.0).to(err.dtype))
    i = int(ratio.argmax())
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ratio.shape))
    return float(ratio.flatten()[i]), idx, float(err[idx]), float(bound[idx])


def _params(cases):
    return [pytest.param(c, m, id=f"{case_id(c)}-{m}") for c in cases for m in c.modes]


def _record(key, r):
    _MAXR[key] = max(_MAXR.get(key, 0.0), r)


@pytest.mark.parametrize("c,mode", _params(rc.rows_cases()))
def test_rows_form(c, mode):
    (t, d), ref = _operands(c, mode), _reference(c, mode)
    got = _run(c, mode, d)
    bound = rc.error_bounds(c, mode, ref, _tdt(mode))
    kind = "zre" if c.pro == "ZRE" else ("prologue" if c.pro != "NONE" else "plain")
    if c.epi != "GNSILU_ADD_FINAL":
        r, idx, e, b = _worst((got["out"].double() - ref["out"]).abs(), bound)
        msg = f"rows_forms[{case_id(c)}-{mode}]: max err / bound {r:.3f} at (image, pixel, channel) {idx}: |got - ref| = {e:.3e}, bound {b:.3e}"
        print("\n" + msg)
        _record(f"{mode} {kind}", r)
        assert r <= 1.0, msg
        return
    bo, bi = rc.final_bounds(c, t, ref, bound, DEV)
    r, idx, e, b = _worst((got["fin_out"].double() - ref["fin_out"]).abs(), bo)
    msg = f"rows_forms[{case_id(c)}-{mode}]: fin_out max err / bound {r:.3f} at (image, pixel) {idx}: |got - ref| = {e:.3e}, bound {b:.3e}"
    ri = 0.0
    if c.fin_mode:
        ri, idx, e, b = _worst((got["fin_img"].double() - ref["fin_img"]).abs(), bi)
        msg += f"; fin_img {ri:.3f} at {idx}: |got - ref| = {e:.3e}, bound {b:.3e}"
    print("\n" + msg)
    _record(f"{mode} final", max(r, ri))
    assert r <= 1.0 and ri <= 1.0, msg


def _same(a, b, what):
    for k in ("out", "fin_out", "fin_img"):
        if a[k] is not None:
            same = _bits(a[k]) == _bits(b[k])
            assert bool(same.all()), (f"{what}: {int((~same).sum())} of {same.numel()} elements of {k} differ, first at "
                                      f"{tuple(int(v) for v in (~same).nonzero()[0])}")


REPEAT = ("s2-half", "final-ddim", "lngate-all-strided", "walk-s2-many-lnmod", "walk-s1-768-many", "walk-zre128-many", "walk-zre256-many",
          "walk-rows32-512-many", "wbatch-lnmod")


@pytest.mark.parametrize("c,mode", _params([c for c in rc.rows_cases() if c.name in REPEAT]))
def test_repeat_launches(c, mode):
    """a launch repeated on fresh buffers reproduces the first result bit for bit"""
    _, d = _operands(c, mode)
    first = _run(c, mode, d)
    for i in range(3):
        _same(first, _run(c, mode, d), f"repeat {i + 1}")


@pytest.mark.parametrize("c,mode", _params(BATCH_CASES))
def test_batch_invariance(c, mode):
    """image 0 of the B = 4 launch (3 workgroups per CU, waves that walk several tiles) and the same image alone (4 per CU, a tile per
    wave): the same bits"""
    t, d = _operands(c, mode, seed=17)
    out4 = _run(c, mode, d)
    assert out4["form"]["wtiles"] > out4["form"]["gx"] * out4["form"]["NT"] // 64
    c1, t1 = rc.batch_slice(c, t, 0)
    out1 = _run(c1, mode, _to_device(t1, mode))
    assert out1["form"]["gx"] != out4["form"]["gx"] and rc.kernel_of(out1["form"]) == rc.kernel_of(out4["form"])
    same = _bits(out1["out"][0]) == _bits(out4["out"][0])
    assert bool(same.all()), (f"{int((~same).sum())} of {same.numel()} elements of image 0 differ between B = 1 and B = 4, first at "
                              f"(pixel, channel) {tuple(int(v) for v in (~same).nonzero()[0])}")


@pytest.mark.parametrize("c,nt", [pytest.param(c, nt, id=case_id(c)) for c, nt in COLUMN_CASES])
def test_column_invariance(c, nt):
    """the first 64 output channels of an 8- or 12-wave launch against the 4-wave launch of those 64 weight rows alone"""
    t, d = _operands(c, "bf16", seed=19)
    wide = _run(c, "bf16", d, expect=dict(NT=nt))
    c64, t64 = rc.column_slice(c, t, 64)
    narrow = _run(c64, "bf16", _to_device(t64, "bf16"), expect=dict(NT=256))
    same = _bits(wide["out"][..., :64]) == _bits(narrow["out"])
    assert bool(same.all()), (f"{int((~same).sum())} of {same.numel()} elements differ between NT {nt} and NT 256, first at (image, "
                              f"pixel, channel) {tuple(int(v) for v in (~same).nonzero()[0])}")


@pytest.mark.parametrize("mode", ["fp32s"])
def test_conv_cols_chunks_agree_with_the_whole_launch(mode):
    """DAEngine.conv_cols computes an fp32s layer in column chunks of its weight matrix: the chunks are the whole launch's bits"""
    from founddiff_amd import _lib as L
    from founddiff_amd.engine import _T, ConvW, DAEngine
    c = rc.COLS32_CASE
    t, d = _operands(c, mode, seed=23)
    whole = _run(c, mode, d)["out"]

    class Bare(DAEngine):
        def __init__(self, m):
            self.mode, self.hip, self.dev, self.buf = m, L.BF16, torch.device(DEV), {}
            self.dt, self.tdt = _T[m]
            self.f32_split = int(m == "fp32s")
    e = Bare(mode)
    cw = ConvW(t["weight"][0, 0], None, e.dev, e.tdt)
    out = torch.full((c.B, c.H, c.W, c.cout), float("nan"), device=DEV)
    K = c.cin
    ok = e.conv_cols(cw, d["in0"], c.B, c.H, c.W, out, c.cout, 2, split=c.split, prologue=L.PRO_LN_MOD, ln_gamma=d["ln_gamma"],
                     ln_beta=d["ln_beta"], ln_eps=rc.EPS, ln_shift=d["ln_mod"], ln_scale=C.c_void_p(d["ln_mod"].data_ptr() + 4 * K),
                     ln_ld=c.ln_ld)
    torch.cuda.synchronize()
    assert ok, "a chunk does not fit the row-GEMM"
    same = _bits(out.view(c.B, -1, c.cout)) == _bits(whole)
    assert bool(same.all()), f"{int((~same).sum())} of {same.numel()} elements differ between the chunks and the whole launch"
