"""The shapes of tests/test_gpu_scan_forms.py, and the fp64 restatement of the fused scan they are compared with.

fd_selective_scan / fd_selective_scan_xproj fan out, by shape alone, into many pieces of device code: the single-pass or the
chunked form, chunk lengths 32 .. 256, one or two channels per lane, 1 / 2 / 4 waves, one or several workgroups per chunk,
three carry kernels or a memset, even or odd images, x_proj inside phase A in bf16 or split fp32.  SCAN_CASES is chosen to
reach every one of them; tests/test_scan_geom_cpu.py asserts that from fd_selective_scan_geom's answers (no GPU), so a case
cannot be dropped, or the launcher's thresholds moved, without the coverage test saying which form lost its test."""
import ctypes as C
from collections import namedtuple

import torch

FD_F32, FD_BF16, LOW_LATENCY, F32_SPLIT = 0, 1, 0x100, 0x200

# modes: 'fp32' (fp32 storage), 'bf16' (the build's 16-bit type), 'fp32s' (fused only: FD_F32 | FD_OPT_F32_SPLIT)
# expect: what fd_selective_scan_geom must answer for this case (asserted in both test modules): nch / cl / nw / wgs / carry /
# last (length of the last chunk) hold for every mode of the case, cpl16 is the 16-bit mode's channels per lane
Case = namedtuple("Case", "D N R H W B ll fused modes expect")


def _c(D, N, R, H, W, B=2, ll=False, fused=False, modes=("fp32", "bf16"), **expect):
    return Case(D, N, R, H, W, B, ll, fused, tuple(modes), expect)


def case_id(c):
    return f"{c.D}-{c.N}-{c.R}-{c.H}x{c.W}" + ("-b1" if c.B == 1 else "") + ("-ll" if c.ll else "") + ("-xproj" if c.fused else "")


SCAN_CASES = [
    # ---- chunked form, throughput set
    _c(64, 16, 8, 91, 93, form=1, cl=64, nch=34, carry=8, nw=1, wgs=1),                   # chunked N 16, odd
    _c(128, 4, 4, 92, 92, form=1, nch=34, last=4, cpl16=2),                               # 16-bit: two channels per lane
    _c(128, 4, 4, 182, 181, form=1, nch=130, carry=0),                                    # odd, two-pass carry
    _c(512, 16, 16, 66, 66, form=1, nch=18, last=1, nw=4, wgs=2),
    _c(512, 32, 16, 66, 64, form=1, cl=64),                                               # chunked N 32
    _c(1024, 4, 2, 182, 182, B=1, form=1, cl=128, nch=65),
    _c(1024, 32, 32, 182, 182, B=1, form=1, cl=128, lds=49152),                           # the widest rows
    _c(1024, 4, 2, 256, 256, B=1, form=1, cl=256),
    # both sides of the carry kernels' boundaries (16 segments of <= 2 / <= 8 / more chunks)
    _c(64, 4, 4, 128, 64, form=1, nch=32, carry=2, last=64),
    _c(64, 4, 4, 66, 126, form=1, nch=33, carry=8),
    _c(64, 4, 4, 256, 128, form=1, nch=128, carry=8),
    _c(64, 4, 4, 172, 192, form=1, nch=129, carry=0),
    # a single chunk: the carry-ins are a memset (L = 63: the last chunk is CL - 1 long; odd)
    _c(64, 8, 4, 18, 13, form=1, nch=1, carry=-1, last=63),
    # last-chunk lengths around the kernel's group length U (16 for N < 16, 8 from N = 16); W = 2: a one-column sub-grid
    _c(128, 8, 4, 130, 2, form=1, cl=64, last=1),
    _c(128, 8, 4, 158, 2, form=1, cl=64, last=15),
    _c(128, 8, 4, 160, 2, form=1, cl=64, last=16),
    _c(128, 8, 4, 162, 2, form=1, cl=64, last=17),
    _c(64, 16, 8, 64, 2, ll=True, form=1, cl=32, nch=1, carry=-1, last=32),
    _c(64, 16, 8, 66, 2, ll=True, form=1, cl=32, last=1),
    _c(64, 16, 8, 78, 2, ll=True, form=1, cl=32, last=7),
    _c(64, 16, 8, 80, 2, ll=True, form=1, cl=32, last=8),
    _c(64, 16, 8, 82, 2, ll=True, form=1, cl=32, last=9),
    # ---- single-pass form: L = 1, 31, 32, 33, 1023, 1024 (the longest ones on odd images too)
    _c(128, 16, 8, 2, 2, form=0),
    _c(128, 16, 8, 62, 2, form=0),
    _c(128, 16, 8, 64, 2, form=0),
    _c(128, 16, 8, 66, 2, form=0),
    _c(128, 16, 8, 66, 62, form=0),
    _c(128, 16, 8, 63, 61, form=0),                                                        # L = 992, odd
    _c(128, 16, 8, 63, 63, form=0),                                                        # L = 1024, odd
    # ---- low-latency set: never single-pass, 32-step chunks, never two channels per lane
    _c(1024, 32, 32, 34, 30, ll=True, form=1, cl=32, last=31, cpl16=1),
    _c(128, 4, 4, 130, 130, ll=True, form=1, nch=133, carry=0, cpl16=1),
    # ---- x_proj inside phase A
    _c(128, 4, 4, 92, 93, fused=True, modes=("bf16", "fp32s"), form=1, cpl16=2),
    _c(256, 8, 8, 183, 182, fused=True, modes=("bf16",), form=1, nch=131, cpl16=1),
    _c(256, 16, 8, 66, 66, fused=True, modes=("bf16",), form=1, cpl16=1),
    _c(256, 16, 8, 32, 32, ll=True, fused=True, modes=("bf16",), form=1, cl=32, cpl16=1),
    _c(256, 8, 8, 66, 66, fused=True, modes=("fp32s",), form=1),
]

# batch invariance (slice i of a B = 3 call == a B = 1 call on that slice, bitwise): one (case, mode) per form
BATCH_CASES = [
    (_c(128, 16, 8, 66, 62, form=0), "bf16"),                          # single-pass
    (_c(128, 4, 4, 92, 92, form=1), "fp32"),                           # chunked, one channel per lane
    (_c(128, 4, 4, 92, 92, form=1, cpl16=2), "bf16"),                  # chunked, two channels per lane
    (_c(128, 4, 4, 92, 93, fused=True, form=1, cpl16=2), "bf16"),      # fused x_proj
]

GEOM_FIELDS = ("form", "cl", "nch", "cpl", "nw", "wgs", "carry", "lds")


def dtype_opts(c, mode):
    base = {"fp32": FD_F32, "bf16": FD_BF16, "fp32s": FD_F32 | F32_SPLIT}[mode]
    return base | (LOW_LATENCY if c.ll else 0)


def seq_len(c):
    return ((c.H + 1) // 2) * ((c.W + 1) // 2)


def geom(lib, c, mode):
    """fd_selective_scan_geom's answer for (case, mode) as a dict (+ 'L', and 'last' = the length of the last chunk)"""
    out = (C.c_int32 * 8)()
    rc = lib.fd_selective_scan_geom(dtype_opts(c, mode), int(c.fused), c.D, c.N, c.R, c.H, c.W, out)
    assert rc == 0, (case_id(c), mode, lib.fd_last_error().decode(errors="replace"))
    g = dict(zip(GEOM_FIELDS, out))
    g["L"] = seq_len(c)
    g["last"] = g["L"] - (g["nch"] - 1) * g["cl"] if g["form"] else 0
    return g


def check_expected(c, mode, g):
    """the geometry the table promises for this case"""
    for k, v in c.expect.items():
        if k == "cpl16":
            if mode == "bf16":
                assert g["cpl"] == v, (case_id(c), mode, k, g)
        else:
            assert g[k] == v, (case_id(c), mode, k, g)
    if mode != "bf16":
        assert g["cpl"] == (1 if g["form"] else 0), (case_id(c), mode, g)


def scan_reference(xc, dtw, dtb, A, Ds, N, R, xdbl=None, xw=None, scan_fn=None, f64=False):
    """The fused scan restated on explicitly gathered operands: EfficientScan gather of xc (B,D,H,W), the x_dbl rows -- given as
    xdbl [4,B,L,R+2N] in the kernel's row layout (row h2 * W2 + w2 whatever the direction), or computed from the x_proj weights
    xw [4,R+2N,D] -- dt_proj, the sequential scan `scan_fn` (oracle.nets.selective_scan / selective_scan_f64) and the
    EfficientMerge scatter.  f64: the einsums in fp64 as well.  Returns (y (B,D,H,W), x_dbl rows [4,B,L,CD] in the row layout or
    None when they were given)."""
    from oracle import nets
    scan_fn = scan_fn or (nets.selective_scan_f64 if f64 else nets.selective_scan)
    B, D, H, W = xc.shape
    CD = R + 2 * N
    H2, W2 = (H + 1) // 2, (W + 1) // 2
    Lq = H2 * W2
    xs = nets.efficient_scan(xc)                                   # (B,4,D,L) in scan order, zero-padded when odd
    up = (lambda t: t.double()) if f64 else (lambda t: t)
    xd_rows = None
    if xw is not None:
        xd_scan = torch.einsum("bkdl,kcd->bklc", up(xs), up(xw))   # rows in scan order
        # x_dbl rows are stored at row index h2 * W2 + w2 whatever the direction's scan order
        xd_rows = torch.stack([xd_scan[:, 0], xd_scan[:, 1].reshape(B, W2, H2, CD).transpose(1, 2).reshape(B, Lq, CD),
                               xd_scan[:, 2], xd_scan[:, 3].reshape(B, W2, H2, CD).transpose(1, 2).reshape(B, Lq, CD)], 0)
    else:
        xd = xdbl.permute(1, 0, 2, 3).reshape(B, 4, H2, W2, CD)
        xd_scan = torch.stack([xd[:, 0].reshape(B, Lq, CD), xd[:, 1].transpose(1, 2).reshape(B, Lq, CD),
                               xd[:, 2].reshape(B, Lq, CD), xd[:, 3].transpose(1, 2).reshape(B, Lq, CD)], 1)
        xd_scan = up(xd_scan)
    dts = torch.einsum("bklr,kdr->bkdl", xd_scan[..., :R], up(dtw))
    Bs = xd_scan[..., R:R + N].permute(0, 1, 3, 2).contiguous()
    Cs = xd_scan[..., R + N:].permute(0, 1, 3, 2).contiguous()
    ys = scan_fn(xs.reshape(B, 4 * D, Lq), dts.reshape(B, 4 * D, Lq), A, Bs, Cs, Ds, dtb.reshape(-1))
    ref = nets.efficient_merge(ys.view(B, 4, D, Lq), H, W).view(B, D, H, W)
    return ref, xd_rows
