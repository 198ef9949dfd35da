"""outer_conv_train.init_conv_fn / final_conv_fn (csrc/fd_outer_train.hip) against float64 torch on the CPU.  Gates as in
tests/test_gpu_resblock_train.py: rel_err = max |a - b| / max |b| below 1e-5 for forward outputs, 1e-4 for activation gradients,
1e-3 for parameter gradients.

Sizes of init_conv_fn: the forward tile is 8 x 32 pixels, the weight gradient's 4 x 32 (Cin 2, Cout a multiple of 64) or 8 x 32, one
partial per range of tiles.  16 x 16 is one tile per slice; 5 x 9 is smaller than the 7 x 7 window, every tap meets a border; 40 x 72
is 5 (10) x 3 tiles per slice, partly filled, and more than one partial per output, so the sums run.  Up to there a range is one
tile.  A workgroup takes several tiles in turn -- the path of every real training shape -- once there are more than
1024 / (Cout / 64 or 32) tiles: 2 x 300 x 222 at Cout 64 is 1050 tiles of 4 x 32 against 1024 (Cin 2) and 532 of 8 x 32 against 512
(Cin 3), two tiles per range, the last column of tiles and (Cin 3) the last row partly filled, and with 525 tiles per slice at Cin 2
one range holds the last tile of slice 0 and the first of slice 1.
Sizes of final_conv_fn: 16 pixels per workgroup forward, 1024 per partial backward, the partials summed 32 at a time and then the
groups: 3 x 5 ends inside a workgroup, 1 x 96 x 96 is nine partials in one group, 1 x 192 x 192 is 36 in two groups (both levels of
the sum), a channel slice of a wider tensor is read in place."""
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err

pytestmark = pytest.mark.gpu
OUT, ACT, PAR = 1e-5, 1e-4, 1e-3


def _report(what, errs):
    print(f"[measured] {what}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))


def _init_case(cin, cout, B, H, W, seed=0):
    g = torch.Generator().manual_seed(seed + 131 * cin + cout + 7 * H + W)
    x = torch.randn(B, cin, H, W, generator=g)
    w = torch.randn(cout, cin, 7, 7, generator=g) / 7.0
    b = torch.randn(cout, generator=g)
    dout = torch.randn(B, H, W, cout, generator=g)
    return x, w, b, dout


def _init_ref(x, w, b, dout):
    w64, b64 = w.double().requires_grad_(), b.double().requires_grad_()
    out = F.conv2d(x.double(), w64, b64, padding=3).permute(0, 2, 3, 1)
    out.backward(dout.double())
    return out.detach(), w64.grad, b64.grad


def _init_run(x, w, b, dout):
    from founddiff_amd.outer_conv_train import init_conv_fn
    xd, wd, bd = x.cuda(), w.cuda().requires_grad_(), b.cuda().requires_grad_()
    keep = [t.detach().clone() for t in (xd, wd, bd)]
    dd = dout.cuda()
    keep.append(dd.clone())
    out = init_conv_fn(xd, wd, bd)
    out.backward(dd)
    torch.cuda.synchronize()
    assert all(torch.equal(a.detach(), k) for a, k in zip((xd, wd, bd, dd), keep)), "an input was overwritten"
    return out.detach(), wd.grad, bd.grad


@pytest.mark.parametrize("cin", [2, 3])
@pytest.mark.parametrize("cout", [32, 64])
@pytest.mark.parametrize("H,W", [(16, 16), (5, 9), (40, 72)])
def test_init_conv_against_float64(cin, cout, H, W):
    _init_against_float64(cin, cout, H, W)


@pytest.mark.parametrize("cin", [2, 3])
def test_init_conv_several_tiles_per_workgroup(cin):
    _init_against_float64(cin, 64, 300, 222)


def _init_against_float64(cin, cout, H, W):
    case = _init_case(cin, cout, 2, H, W)
    ref = _init_ref(*case)
    got = _init_run(*case)
    assert got[0].shape == (2, H, W, cout) and got[1].shape == (cout, cin, 7, 7) and got[2].shape == (cout,)
    errs = {k: rel_err(g.cpu(), r) for k, g, r in zip(("out", "dweight", "dbias"), got, ref)}
    _report(f"init_conv_fn Cin {cin} Cout {cout} {H}x{W}", errs)
    assert errs["out"] < OUT and errs["dweight"] < PAR and errs["dbias"] < PAR, errs


def test_init_conv_x_is_data():
    from founddiff_amd.outer_conv_train import init_conv_fn
    x, w, b, _ = _init_case(2, 32, 1, 8, 8)
    with pytest.raises(RuntimeError, match="init_conv_fn.*x is data"):
        init_conv_fn(x.cuda().requires_grad_(), w.cuda().requires_grad_(), b.cuda())


def _final_case(C, B, H, W, ld=None, off=0, seed=0):
    g = torch.Generator().manual_seed(seed + C + 7 * H + W)
    wide = torch.randn(B, H, W, ld or C, generator=g)
    w = torch.randn(1, C, 1, 1, generator=g) / C ** 0.5
    b = torch.randn(1, generator=g)
    dout = torch.randn(B, 1, H, W, generator=g)
    return wide, off, C, w, b, dout


def _final_ref(wide, off, C, w, b, dout):
    x64 = wide[..., off:off + C].double().requires_grad_()
    w64, b64 = w.double().requires_grad_(), b.double().requires_grad_()
    out = F.conv2d(x64.permute(0, 3, 1, 2), w64, b64)
    out.backward(dout.double())
    return out.detach(), x64.grad, w64.grad, b64.grad


def _final_run(wide, off, C, w, b, dout):
    from founddiff_amd.outer_conv_train import final_conv_fn
    wd = wide.cuda()
    x = wd[..., off:off + C].detach().requires_grad_()               # a leaf over the wide tensor's memory: a slice is read in place
    assert x.data_ptr() == wd.data_ptr() + 4 * off and x.is_contiguous() == (wd.shape[3] == C)
    ww, bb, dd = w.cuda().requires_grad_(), b.cuda().requires_grad_(), dout.cuda()
    keep = [t.detach().clone() for t in (wd, ww, bb, dd)]
    out = final_conv_fn(x, ww, bb)
    out.backward(dd)
    torch.cuda.synchronize()
    assert all(torch.equal(a.detach(), k) for a, k in zip((wd, ww, bb, dd), keep)), "an input was overwritten"
    return out.detach(), x.grad, ww.grad, bb.grad


@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("B,H,W,ld,off", [(2, 16, 16, None, 0), (2, 3, 5, None, 0), (2, 16, 16, 192, 64), (1, 96, 96, None, 0),
                                          (1, 192, 192, None, 0)])
def test_final_conv_against_float64(C, B, H, W, ld, off):
    if ld is not None:
        ld, off = 3 * C, C                           # the middle third of a wider tensor
    case = _final_case(C, B, H, W, ld, off)
    ref = _final_ref(*case)
    got = _final_run(*case)
    assert got[0].shape == (B, 1, H, W) and got[1].shape == (B, H, W, C) and got[2].shape == (1, C, 1, 1) and got[3].shape == (1,)
    errs = {k: rel_err(g.cpu(), r) for k, g, r in zip(("out", "dx", "dweight", "dbias"), got, ref)}
    _report(f"final_conv_fn C {C} {B}x{H}x{W} ld {ld} off {off}", errs)
    assert errs["out"] < OUT and errs["dx"] < ACT and errs["dweight"] < PAR and errs["dbias"] < PAR, errs


def test_deterministic_and_batch_invariant():
    """two runs give the same bits; slice 1 alone equals slice 1 of the batch, in out and in dx"""
    for cin, H, W in ((2, 40, 72), (2, 300, 222), (3, 300, 222)):        # one tile per workgroup, and several
        case = _init_case(cin, 64, 2, H, W, seed=3)
        a, b = _init_run(*case), _init_run(*case)
        assert all(torch.equal(p, q) for p, q in zip(a, b))
        x, w, bias, dout = case
        one = _init_run(x[1:], w, bias, dout[1:])
        assert torch.equal(one[0][0], a[0][1])
    for ld, off, H, W in ((None, 0, 24, 40), (192, 64, 24, 40), (None, 0, 192, 192)):
        case = _final_case(64, 2, H, W, ld, off, seed=3)
        a, b = _final_run(*case), _final_run(*case)
        assert all(torch.equal(p, q) for p, q in zip(a, b))
        wide, off, C, w, bias, dout = case
        one = _final_run(wide[1:], off, C, w, bias, dout[1:])
        assert torch.equal(one[0][0], a[0][1]) and torch.equal(one[1][0], a[1][1])


def test_argument_errors_fire_before_a_launch():
    from founddiff_amd import _lib as L
    from founddiff_amd.outer_conv_train import final_conv_fn, init_conv_fn
    x, w, b, _ = (t.cuda() for t in _init_case(2, 32, 1, 8, 8))
    wide, _, _, fw, fb, _ = _final_case(64, 1, 4, 4)
    fx, fw, fb = wide.cuda(), fw.cuda(), fb.cuda()
    L.lib()
    L.TRACE = []
    try:
        for bad, match in (((x.cpu(), w, b), "init_conv_fn: x must live on the GPU"),
                           ((x, w.double(), b), "init_conv_fn: weight must be float32"),
                           ((x, torch.zeros(48, 2, 7, 7).cuda(), torch.zeros(48).cuda()), "init_conv_fn: unsupported shape.*Cout=48"),
                           ((x, w[:, :1], b), "init_conv_fn: inconsistent shapes"),
                           (([1.0], w, b), "init_conv_fn: x must be a tensor")):
            with pytest.raises(RuntimeError, match=match):
                init_conv_fn(*bad)
        for bad, match in (((fx.cpu(), fw, fb), "final_conv_fn: x must live on the GPU"),
                           ((fx.long(), fw, fb), "final_conv_fn: x must be float32"),
                           ((fx[..., :6], fw[:, :6], fb), "final_conv_fn: unsupported shape C=6"),
                           ((fx, fw[:, :32], fb), "final_conv_fn: inconsistent shapes")):
            with pytest.raises(RuntimeError, match=match):
                final_conv_fn(*bad)
        assert L.TRACE == [], L.TRACE
    finally:
        L.TRACE = None
