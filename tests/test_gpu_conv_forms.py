"""Every tile and loader form of the generic implicit-GEMM convolution (conv_igemm_kernel, csrc/fd_conv.hip) against an fp64 restatement.

The cases are tests/conv_cases.CONV_CASES; tests/test_conv_forms_cpu.py asserts, without a GPU, that they reach all 28 instantiations
(tile ids 0 .. 6 x bf16 pointwise loader / bf16 general gather / fp32 / split fp32) and the M / N / K edges, layouts and epilogue paths
of its coverage list.  The reference is conv_cases.conv_reference: explicit gather, F.conv2d in fp64, the epilogue in fp64.

Which test pins which id of fd_conv_kernel_id (probe="kid" / "form" / True before the launch it compares with a reference):
  0, 1, 2, 3, 4, 5, 6   test_conv_form here (fd_conv_form: the id and the loader), every one in all four element forms
  5, 7                  test_gpu_kernels.py::test_pointwise_gemm_256_tile; 7 also test_gpu_round6.py::test_pointwise_gemm_gate_table_batch_groups
  10, 17                test_gpu_rows_forms.py::test_rows_form (fd_gemm_rows_form: every instantiation, workgroup size and tile walk of both)
  10                    also test_gpu_kernels.py::test_row_gemm_fused_prologues, test_row_gemm_final_conv_ddim_epilogue (fd_conv_prologue_ok)
  17                    also test_gpu_round6.py::test_row_gemm_fp32_storage_split_bf16
  11                    test_gpu_kernels.py::test_conv3x3_halo, test_conv3x3_weights_in_registers (its 128-channel twin)
  12                    test_gpu_kernels.py::test_conv3x3_fp8_weights
  13                    test_gpu_kernels.py::test_conv3x3_weights_in_registers
  14                    test_gpu_round5.py::test_conv3x3_upsample_as_four_2x2
  15                    test_gpu_round5.py::test_conv3x3_split_bf16_halo
  16                    test_gpu_round5.py::test_conv3x3_upsample_four_2x2_split_bf16

Comparison: element by element, |got - ref| <= bound with (conv_cases.error_bounds)
    bound = u_out |ref| + L c_mode S + 2^-20 (|ref| + |addend|)
u_out the unit roundoff of the stored type, S the same convolution of |x| with |w| (+ |bias|), L the epilogue's Lipschitz factor,
c_mode = (K + 8) 2^-24 (+ 2^-14 in the split mode).  Nothing is tuned to the kernel; no term had to be added.
Largest err / bound over the table, recorded on an MI355X (a record of the margin, not a gate): default build bf16 0.995, fp32 0.080,
fp32s 0.121; binary16 build 0.991.  (In the 16-bit modes the store rounding alone reaches 0.99 of the bound at elements just above a
power of two -- u_out is exactly that rounding -- so what is left there for the contraction is the S term; the fp32 modes show the
contraction's own margin.)  Largest band-sum error / tolerance: 0.012 for the sums, 0.018 for the sums of squares.

Beyond the comparison, on every case: the output is pre-filled with NaN and every element the convolution owns comes back finite; the
slack channels of a wider output row and a guard row behind the last pixel of the last direction hold a sentinel and come back with
their own bits; the GroupNorm sums are exactly B . fd_conv_mtiles . Cout . 2 floats, NaN-filled, every one written, and a guard behind
them untouched.  Each band's sum and sum of squares is compared with the fp64 band sums of the reference output within
64 . 2^-24 . sum |val| (sum val^2) for the fp32 summation plus the element bound (before the store rounding) summed over the band.

On top of the table, bit for bit (torch.equal): one image computed alone and in a batch that moves the launch to another tile
(ids 2 -> 4, 2 -> 5); the pointwise loader against the general gather on the same problem; a launch repeated three times."""
import ctypes as C

import pytest
import torch

import conv_cases as cc
from conftest import HB, use_half_build
from conv_cases import BATCH_CASES, CONV_CASES, PW_GENERAL_CASES, case_id, expected_form

pytestmark = pytest.mark.gpu

GUARD = 64                    # floats behind the GroupNorm sums
SENTINEL = -12345.0           # exact in fp32, finite in both 16-bit types: slack and guards are compared with their own bits


@pytest.fixture(scope="module", params=["bf16-build", "fp16-build"], autouse=True)
def half_build(request):
    """every test of this module once per build of the library (conftest.use_half_build)"""
    use_half_build(request.param == "fp16-build")
    _CACHE.clear()
    yield request.param
    use_half_build(False)
    if _MAXR:
        print(f"\nconv_forms[{request.param}]: largest err / bound per mode: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(_MAXR.items())))
    _MAXR.clear()


@pytest.fixture(autouse=True)
def _default_build_only(request, half_build):
    """the fp32-storage and split modes belong to the default build: not repeated on the binary16 one"""
    if half_build == "fp16-build":
        mode = getattr(request.node, "callspec", None) and request.node.callspec.params.get("mode")
        if mode in ("fp32", "fp32s"):
            pytest.skip("default build only")


_CACHE = {}       # the operands (and the reference) of the case that ran last: its modes follow each other, fp32 and fp32s share both
_MAXR = {}        # mode -> largest err / bound seen (a record, not a gate)
_FAULTED = []     # the launch that raised, if one did: the device may be in no state to go on


def _operands(c, mode, seed=11):
    tdt = HB.t if mode == "bf16" else torch.float32
    key = (case_id(c), c.B, tdt, seed)
    if _CACHE.get("key") != key:
        rq = (lambda t: t.to(HB.t).float()) if mode == "bf16" else (lambda t: t)
        _CACHE.clear()
        _CACHE.update(key=key, t=cc.make_inputs(c, rq, seed))
    return _CACHE["t"]


def _reference(c, mode):
    t = _operands(c, mode)
    if "ref" not in _CACHE:
        _CACHE["ref"] = cc.conv_reference(c, t)
    return _CACHE["ref"]


def _bits(x):
    return x.view(torch.int32 if x.dtype == torch.float32 else torch.int16)


def _run(c, mode, t):
    """one fd_conv2d launch on guarded, NaN-filled buffers -> (out [ndir, B, OH*OW, Cout] in its stored type, sums [B, bands, Cout, 2]
    or None), both on the GPU; the dispatch pin, the guards and the finiteness of what was written are asserted here"""
    from founddiff_amd import _lib as L
    if _FAULTED:
        pytest.fail(f"the launch of {_FAULTED[0]} raised: nothing more is launched from this module")
    lib = L.lib()
    tdt = HB.t if mode == "bf16" else torch.float32
    odt = torch.float32 if c.out_f32 else tdt
    P, rows = cc.ohw(c), c.ndir * c.B * cc.ohw(c)
    d = {k: v.to("cuda", tdt if k in ("in0", "in1", "weight", "res", "h") else torch.float32).contiguous() for k, v in t.items()}
    buf = torch.full((rows + 1, c.ldo), float("nan"), device="cuda", dtype=odt)            # + a guard row
    buf[:, :c.offo] = SENTINEL
    buf[:, c.offo + c.cout:] = SENTINEL
    buf[rows:] = SENTINEL
    before = buf.clone()
    ptrs = {k: v.data_ptr() for k, v in d.items()}
    ptrs["out"] = buf.data_ptr()
    st = None
    if c.stats:
        nst = c.B * lib.fd_conv_mtiles(c.OH, c.OW) * c.cout * 2
        assert nst == c.B * cc.bands(c) * c.cout * 2
        st = torch.full((nst + GUARD,), float("nan"), device="cuda")
        st[nst:] = SENTINEL
        ptrs["stats"] = st.data_ptr()
    p = cc.params_for(c, mode, ptrs)
    got = int(lib.fd_conv_form(C.byref(p)))
    assert got == expected_form(c, mode), f"{case_id(c)}-{mode}: form {got:#x}, the table says {expected_form(c, mode):#x}"
    try:
        L.call("fd_conv2d", C.byref(p), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    except Exception:
        _FAULTED.append(f"{case_id(c)}-{mode}")
        raise
    own = buf[:rows, c.offo:c.offo + c.cout]
    assert bool(torch.isfinite(own).all()), "out: elements left unwritten (NaN pre-fill) or non-finite"
    out = own.reshape(c.ndir, c.B, P, c.cout).clone()
    buf[:rows, c.offo:c.offo + c.cout] = 0
    before[:rows, c.offo:c.offo + c.cout] = 0
    assert torch.equal(_bits(buf), _bits(before)), "slack channels or the guard row behind the output were written"
    if c.stats:
        assert bool((st[nst:] == SENTINEL).all()), "the guard behind the GroupNorm sums was written"
        st = st[:nst].view(c.B, cc.bands(c), c.cout, 2)
        assert bool(torch.isfinite(st).all()), "GroupNorm sums: entries left unwritten (NaN pre-fill) or non-finite"
    return out, st


def _worst(err, bound):
    """largest err / bound and where; a bound of exactly 0 (zero-filled operand rows: ref, S and addend all 0) admits err = 0 only"""
    ratio = torch.where(bound > 0, err / bound, torch.where(err > 0, float("inf"), 0.0).to(err.dtype))
    i = int(ratio.argmax())
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ratio.shape))
    return float(ratio.flatten()[i]), idx


def _params(cases):
    return [pytest.param(c, m, id=f"{case_id(c)}-{m}") for c in cases for m in c.modes]


@pytest.mark.parametrize("c,mode", _params(CONV_CASES))
def test_conv_form(c, mode):
    t, ref = _operands(c, mode), _reference(c, mode)
    out, st = _run(c, mode, t)
    bound, pre = cc.error_bounds(c, mode, ref, out.dtype)
    err = (out.double().cpu() - ref["out"]).abs()
    r, idx = _worst(err, bound)
    msg = f"conv_forms[{case_id(c)}-{mode}]: max err / bound {r:.3f} at (dir, image, pixel, channel) {idx}"
    if c.stats:
        got = st.double().cpu()
        tol_s = 64 * 2.0 ** -24 * ref["abs"] + cc.band_sum(c, pre.expand_as(ref["out"]))
        tol_q = 64 * 2.0 ** -24 * ref["sq"] + cc.band_sum(c, (2 * ref["out"].abs() * pre + pre * pre).expand_as(ref["out"]))
        rs, ids = _worst((got[..., 0] - ref["sum"]).abs(), tol_s)
        rq, idq = _worst((got[..., 1] - ref["sq"]).abs(), tol_q)
        msg += f"; sums {rs:.3f} at (image, band, channel) {ids}, sums of squares {rq:.3f} at {idq}"
    print("\n" + msg)
    _MAXR[mode] = max(_MAXR.get(mode, 0.0), r)
    assert r <= 1.0, msg + f": |got - ref| = {float(err[idx]):.3e} > bound {float(bound.expand_as(err)[idx]):.3e}"
    if c.stats:
        assert rs <= 1.0 and rq <= 1.0, msg


@pytest.mark.parametrize("c,mode", _params(CONV_CASES))
def test_repeat_launches(c, mode):
    """a launch repeated on fresh buffers reproduces the first result bit for bit, sums included"""
    t = _operands(c, mode)
    out0, st0 = _run(c, mode, t)
    for i in range(3):
        out, st = _run(c, mode, t)
        assert torch.equal(_bits(out), _bits(out0)), f"repeat {i + 1}: the output differs from the first launch"
        if c.stats:
            assert torch.equal(st, st0), f"repeat {i + 1}: the GroupNorm sums differ from the first launch"


@pytest.mark.parametrize("mode", cc.BATCH_MODES)
@pytest.mark.parametrize("c,kid1", [pytest.param(c, k, id=case_id(c)) for c, k in BATCH_CASES])
def test_batch_invariance_across_tiles(c, kid1, mode):
    """csrc/fd_conv.hip: "every output element accumulates its K tiles in the same order whatever the tile shape (bitwise identical
    results)".  One per-image problem at B = 2 (the 8-wave tile the table names) and each image alone (the 64 x 128 tile)."""
    t = _operands(c, mode, seed=17)
    out2, _ = _run(c, mode, t)
    for i in range(c.B):
        c1, t1 = cc.batch_slice(c, t, i)
        out1, _ = _run(c1._replace(expect=dict(c.expect, kid=kid1)), mode, t1)
        assert torch.equal(_bits(out1[:, 0]), _bits(out2[:, i])), f"image {i}: tile {kid1} at B = 1 and tile {c.expect['kid']} at B = 2 differ"


@pytest.mark.parametrize("c", [pytest.param(c, id=case_id(c)) for c in PW_GENERAL_CASES])
def test_pointwise_loader_against_general_gather(c):
    """csrc/fd_conv.hip: "pointwise fast path: same tiles, same K order, same results".  The same 1x1 problem through the pointwise
    loader (one source) and through the general gather (the K axis split over two sources at channel 72), on both builds.
    (GNSILU_ADD failed here at first: the staged epilogue computed (h - mean) * rstd * gamma + beta, the direct one
    (h * rstd - mean * rstd) * gamma + beta -- 1 .. 85 stored elements per launch differed in their last bit.  Both now call
    fd_gn_silu_add8, csrc/fd_common.h.)"""
    t = _operands(c, "bf16", seed=19)
    out_pw, _ = _run(c, "bf16", t)
    c2, t2 = cc.split_sources(c, t)
    out_gen, _ = _run(c2, "bf16", t2)
    same = _bits(out_pw) == _bits(out_gen)
    assert bool(same.all()), (f"{int((~same).sum())} of {same.numel()} elements differ between the loaders, first at (dir, image, pixel, "
                              f"channel) {tuple(int(v) for v in (~same).nonzero()[0])}")
