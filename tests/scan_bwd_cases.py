"""The shapes of tests/test_gpu_scan_bwd_cases.py, the fp64 restatements they are compared with, and the gate they are held to.

The two scan backwards -- fd_cross_scan_bwd_f32 / _nhwc_f32 (csrc/fd_cross_scan_bwd.hip) and fd_selective_scan_bwd_f32
(csrc/fd_scan_bwd.hip) -- fan out, by shape alone, into 40 template instantiations, two tile lengths, one to sixteen channel or
row splits, ragged last tiles, lanes and x_proj blocks, and directions that are all padding.  CS_CASES and SB_CASES are chosen to
reach every one of them; tests/test_scan_bwd_cases_cpu.py asserts that from fd_cross_scan_bwd_geom / fd_selective_scan_bwd_geom
(the launchers' own layout functions, no GPU), so a case cannot be dropped, or a threshold moved, without the coverage test naming
the edge that lost its test.  Each case's `expect` is what the query must answer for it, asserted in both test modules.

To add a case: append it with the geometry you expect, add the edge it stands for to cs_gaps / sb_gaps below (a case no edge needs
fails test_every_case_is_needed), run the GPU module with FD_RECORD_SCAN_BWD_ERRORS=<path> on an MI355X and merge the new keys into
tests/golden/scan_bwd_measured_errors.json."""
import ctypes as C
import json
import os
from collections import namedtuple

import torch
import torch.nn.functional as F

from scan_bwd_ref import scan_grads_f64

HOT_EVERY = 16         # every 16th channel: delta + bias in 21 .. 25, the v > 20 branch of softplus and of its derivative
HOT_BIAS = 23.0

# ---- the cross-scan backward -------------------------------------------------------------------------------------------------
CsCase = namedtuple("CsCase", "D N R H W B expect")
CS_FIELDS = ("E", "tile", "L", "ntiles", "last", "S", "nxb", "lds")
LAYOUTS = ("nchw", "nhwc")


def _cs(D, N, R, H, W, B=2, **expect):
    return CsCase(D, N, R, H, W, B, expect)


def cs_id(c):
    return f"{c.D}-{c.N}-{c.R}-{c.H}x{c.W}" + ("-b1" if c.B == 1 else "")


CS_CASES = [
    # ---- E = 4 (R + 2N <= 24): 256-position tiles, a lane walks 4 positions
    _cs(64, 4, 2, 1, 1, E=4, L=1, ntiles=1, S=1),                       # three directions are all padding
    _cs(64, 4, 4, 7, 1, E=4, L=4),                                      # W = 1
    _cs(64, 4, 8, 1, 9, E=4, L=5),                                      # H = 1
    _cs(64, 4, 4, 5, 4, E=4, L=6),                                      # odd H alone
    _cs(128, 4, 16, 34, 30, E=4, L=255, ntiles=1, S=2),                 # R + 2N = 24; one tile of TILE - 1
    _cs(128, 8, 2, 32, 32, E=4, L=256, ntiles=1, last=256, nxb=1),      # exactly one tile and one x_proj block
    _cs(64, 8, 4, 514, 2, E=4, L=257, ntiles=2, last=1, nxb=2),         # last tile and last x_proj block of one row
    _cs(64, 8, 8, 33, 31, E=4, L=272, ntiles=2, last=16),               # R + 2N = 24, odd
    _cs(128, 4, 4, 63, 65, E=4, L=1056, ntiles=5, last=32, S=2),        # five tiles, odd
    _cs(256, 4, 4, 17, 15, E=4, L=72, ntiles=1, S=4),                   # S = 4 on a partial tile
    # ---- E = 1: 64-position tiles
    _cs(64, 4, 32, 18, 13, E=1, L=63, ntiles=1),
    _cs(64, 8, 16, 16, 16, E=1, L=64, ntiles=1, last=64),
    _cs(64, 8, 32, 130, 2, E=1, L=65, ntiles=2, last=1),
    _cs(128, 16, 2, 15, 13, E=1, L=56, S=2),
    _cs(64, 16, 4, 2, 2, E=1, L=1),
    _cs(64, 16, 16, 31, 33, E=1, L=272, ntiles=5, last=16, nxb=2),
    _cs(64, 16, 32, 9, 7, E=1, L=20),
    _cs(64, 32, 2, 66, 62, E=1, L=1023, ntiles=16, last=63),
    _cs(64, 32, 4, 63, 63, E=1, L=1024, ntiles=16, last=64),
    _cs(64, 32, 8, 66, 64, E=1, L=1056, ntiles=17, last=32),
    # ---- channel splits: both sides of the 512-workgroup threshold, S = 8, 16, and S held by the workgroup count
    _cs(128, 16, 8, 254, 128, B=1, E=1, ntiles=127, S=2),
    _cs(128, 16, 8, 256, 128, B=1, E=1, ntiles=128, S=1),
    _cs(512, 32, 16, 16, 16, E=1, ntiles=1, S=8),
    _cs(1024, 32, 32, 8, 8, B=1, E=1, ntiles=1, S=16),
    _cs(512, 16, 16, 64, 128, B=1, E=1, ntiles=32, S=4),
]

# slice i of a B = 3 call is bitwise the B = 1 call (y and dx), in both layouts
CS_BATCH_IDS = ("128-4-16-34x30", "256-4-4-17x15", "64-16-16-31x33")


def cs_geom(lib, c):
    out = (C.c_int32 * 8)()
    rc = lib.fd_cross_scan_bwd_geom(c.B, c.H, c.W, c.D, c.N, c.R, out)
    assert rc == 0, (cs_id(c), lib.fd_last_error().decode(errors="replace"))
    return dict(zip(CS_FIELDS, out))


def check_expected(tag, expect, g):
    for k, v in expect.items():
        assert g[k] == v, (tag, k, v, g)


def cs_gaps(rows):
    """the edges of the cross-scan backward that `rows` -- (case, geometry) pairs -- do NOT reach, by name"""
    gaps = []

    def need(name, pred):
        if not any(pred(c, g) for c, g in rows):
            gaps.append(name)

    for N in (4, 8, 16, 32):
        for R in (2, 4, 8, 16, 32):
            need(f"the instantiation N = {N}, R = {R}", lambda c, g: (c.N, c.R) == (N, R))
    need("R + 2N = 24, the widest row at 4 positions per lane", lambda c, g: c.R + 2 * c.N == 24 and g["E"] == 4)
    for E in (1, 4):
        need(f"E = {E}", lambda c, g: g["E"] == E)
        need(f"E = {E}: L = 1", lambda c, g: g["E"] == E and g["L"] == 1)
        for nm, ln in (("1", lambda g: 1), ("TILE - 1", lambda g: g["tile"] - 1), ("TILE", lambda g: g["tile"])):
            need(f"E = {E}: a single tile of length {nm}", lambda c, g: g["E"] == E and g["ntiles"] == 1 and g["last"] == ln(g))
        need(f"E = {E}: interior tiles (three or more)", lambda c, g: g["E"] == E and g["ntiles"] >= 3)
    for nm, ln in (("1", lambda g: 1), ("TILE - 1", lambda g: g["tile"] - 1), ("TILE", lambda g: g["tile"])):
        need(f"a last tile of length {nm} behind full tiles", lambda c, g: g["ntiles"] > 1 and g["last"] == ln(g))
    need("E = 4: a last lane with 1 - 3 of its 4 positions, behind full tiles",
         lambda c, g: g["E"] == 4 and g["ntiles"] > 1 and g["last"] % 4)
    need("one x_proj block", lambda c, g: g["nxb"] == 1 and g["L"] == 256)
    need("a last x_proj block of one row", lambda c, g: g["nxb"] == 2 and g["L"] == 257)
    need("E = 1: two x_proj blocks", lambda c, g: g["E"] == 1 and g["nxb"] == 2 and g["ntiles"] < 8)
    for S in (1, 2, 4, 8, 16):
        need(f"S = {S}", lambda c, g: g["S"] == S)
    need("S = 2 on a partial tile (dxp -> cs_sum_kernel)", lambda c, g: g["S"] == 2 and g["last"] < g["tile"])
    need("S = 4 on a partial tile (dxp -> cs_sum_kernel)", lambda c, g: g["S"] == 4 and g["last"] < g["tile"])
    # the 4 ntiles S < 512 threshold from both sides, at equal (D, N, R)
    below = {(c.D, c.N, c.R) for c, g in rows if g["S"] == 2 and 4 * (g["ntiles"] + 1) >= 512 and c.D % 256}
    above = {(c.D, c.N, c.R) for c, g in rows if g["S"] == 1 and 4 * g["ntiles"] == 512 and c.D % 128 == 0}
    if not below:
        gaps.append("one tile below the 512-workgroup threshold (S = 2)")
    if not above:
        gaps.append("at the 512-workgroup threshold (S = 1 where d_inner would allow 2)")
    if below and above and not below & above:
        gaps.append("both sides of the 512-workgroup threshold at equal (d_inner, N, R)")
    need("S > 1 stopped by the workgroup count, not by divisibility",
         lambda c, g: g["S"] > 1 and 4 * g["ntiles"] * g["S"] >= 512 and c.D % (128 * g["S"]) == 0)
    need("H = 1", lambda c, g: c.H == 1 and c.W > 1)
    need("W = 1", lambda c, g: c.W == 1 and c.H > 1)
    need("odd H alone", lambda c, g: c.H % 2 == 1 and c.W % 2 == 0)
    need("odd W alone", lambda c, g: c.H % 2 == 0 and c.W % 2 == 1)
    need("odd H and W over several tiles", lambda c, g: c.H % 2 == 1 and c.W % 2 == 1 and g["ntiles"] > 1)
    ids = {cs_id(c) for c, g in rows}
    for i in CS_BATCH_IDS:
        if i not in ids:
            gaps.append(f"the batch-invariance case {i}")
    return gaps


# ---- the reference-layout backward ---------------------------------------------------------------------------------------------
SbCase = namedtuple("SbCase", "batch KD K N L softplus has_D has_bias nrows expect")
SB_FIELDS = ("ntiles", "tgroups", "last", "S", "NC", "rps", "Dg")


def _sb(batch, KD, K, N, L, softplus=True, has_D=True, has_bias=True, nrows=1, **expect):
    return SbCase(batch, KD, K, N, L, softplus, has_D, has_bias, nrows, expect)


def sb_id(c):
    return f"{c.batch}-{c.KD}-{c.K}-{c.N}-{c.L}"


SB_CASES = [
    _sb(1, 4, 4, 1, 1, ntiles=1, S=1, NC=4, Dg=1),                                         # one row, one state, one position
    _sb(2, 24, 4, 3, 255, softplus=False, has_D=False, has_bias=False, nrows=3, last=255, Dg=6, NC=4),
    _sb(2, 24, 2, 5, 256, has_D=False, nrows=4, ntiles=1, last=256, NC=8),
    _sb(1, 64, 2, 9, 257, nrows=2, ntiles=2, tgroups=1, last=1, S=2, rps=16),              # S held by 16 rows per split
    # (S is the largest power of two with 16 S <= Dg while the workgroups stay below 1024: Dg = 54 gives S = 2, two splits of
    #  27 rows that the four waves do not divide; Dg = 112 gives S = 4)
    _sb(2, 54, 1, 12, 1023, nrows=3, ntiles=4, last=255, S=2, rps=27),
    _sb(1, 112, 1, 16, 1025, softplus=False, nrows=4, ntiles=5, tgroups=2, last=1, S=4, rps=28),
    _sb(2, 64, 4, 4, 2049, has_D=False, has_bias=False, ntiles=9, tgroups=3, S=1, NC=4),
    _sb(1, 40, 1, 33, 300, has_D=False, has_bias=False, nrows=2, ntiles=2, NC=8),
    _sb(1, 8, 2, 256, 70, softplus=False, has_D=False, has_bias=False, Dg=4),
    _sb(1, 20, 2, 15, 513, nrows=2, ntiles=3, last=1, NC=8, Dg=10),                        # N % NC = NC - 1 at NC = 8
    _sb(8, 512, 4, 4, 4096, ntiles=16, tgroups=4, S=2, rps=64),                            # S held by the workgroup count
    _sb(8, 512, 4, 4, 8192, nrows=2, ntiles=32, tgroups=8, S=1),
]


def sb_geom(lib, c):
    out = (C.c_int32 * 8)()
    rc = lib.fd_selective_scan_bwd_geom(c.batch, c.KD, c.K, c.N, c.L, out)
    assert rc == 0, (sb_id(c), lib.fd_last_error().decode(errors="replace"))
    return dict(zip(SB_FIELDS, out))


def sb_gaps(rows):
    """the edges of the reference-layout backward that `rows` do NOT reach, by name"""
    gaps = []

    def need(name, pred):
        if not any(pred(c, g) for c, g in rows):
            gaps.append(name)

    wg = lambda c, g: c.batch * c.K * g["ntiles"]
    need("one row per group, one state, one position", lambda c, g: g["Dg"] == 1 and c.N == 1 and c.L == 1)
    for nm, ln in (("255", 255), ("256", 256)):
        need(f"a single tile of length {nm}", lambda c, g: g["ntiles"] == 1 and g["last"] == ln)
    for nm, ln in (("1", 1), ("255", 255), ("256", 256)):
        need(f"a last tile of length {nm} behind full tiles", lambda c, g: g["ntiles"] > 1 and g["last"] == ln)
    need("tile groups not ragged (ntiles % 4 == 0)", lambda c, g: g["ntiles"] % 4 == 0)
    need("tile groups ragged over two or more groups", lambda c, g: g["ntiles"] % 4 and g["tgroups"] >= 2)
    need("NC = 4 with ragged tile groups", lambda c, g: g["NC"] == 4 and g["ntiles"] % 4 and g["tgroups"] >= 2)
    for NC in (4, 8):
        for nm, rem in (("0", 0), ("1", 1), ("NC - 1", NC - 1)):
            need(f"NC = {NC}: N % NC = {nm}", lambda c, g: g["NC"] == NC and c.N % NC == rem)
    need("N = NC + 1: a second state chunk of one state", lambda c, g: c.N == g["NC"] + 1)
    need("N > 32 in more than two state chunks, the last of one state", lambda c, g: 32 < c.N < 256 and c.N % g["NC"] == 1)
    need("N = 256, the largest accepted", lambda c, g: c.N == 256)
    for S in (1, 2, 4):
        need(f"S = {S}", lambda c, g: g["S"] == S)
    need("S > 1 held by 16 rows per split", lambda c, g: g["S"] > 1 and wg(c, g) * g["S"] < 1024 and 32 * g["S"] > g["Dg"])
    need("S > 1 held by the workgroup count", lambda c, g: g["S"] > 1 and wg(c, g) * g["S"] >= 1024 and 32 * g["S"] <= g["Dg"])
    need("S = 1 held by the workgroup count", lambda c, g: g["S"] == 1 and wg(c, g) >= 1024 and 32 <= g["Dg"])
    need("splits of a row count the four waves do not divide", lambda c, g: g["S"] > 1 and g["rps"] % 4)
    need("rows per group not divisible by 4, several tiles or rows", lambda c, g: g["Dg"] % 4 and g["Dg"] > 1 and c.L == 255)
    need("L % 4 == 0 over two tiles (vector loads, a ragged last tile)", lambda c, g: c.L % 4 == 0 and g["ntiles"] == 2 and g["last"] < 256)
    for n in (1, 2, 3, 4):
        need(f"nrows = {n}", lambda c, g: c.nrows == n)
    if sum(not c.softplus for c, g in rows) < 3:
        gaps.append("softplus off on three cases")
    if sum(not c.has_D and not c.has_bias for c, g in rows) < 3:
        gaps.append("D and delta_bias absent on three cases")
    need("softplus with a bias and without", lambda c, g: c.softplus and not c.has_bias)
    need("no softplus, with D and delta_bias", lambda c, g: not c.softplus and c.has_bias and c.has_D)
    need("delta_bias without D", lambda c, g: c.has_bias and not c.has_D)
    need("B / C 3-D (K = 1)", lambda c, g: c.K == 1)
    return gaps


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def _params(D, N, R, seed):
    """SS2D's initialisation scales (src/emamba2.py: x_proj ~ d_inner^-0.5, dt_proj ~ dt_rank^-0.5, dt bias of a softplus-inverse
    dt in [1e-3, 1e-1], A_logs = log(1..N), Ds = 1), drawn in fp32 so that the oracle's .float() casts are exact"""
    g = torch.Generator().manual_seed(seed)
    dt = torch.exp(torch.rand(4, D, generator=g) * (torch.log(torch.tensor(0.1)) - torch.log(torch.tensor(1e-3)))
                   + torch.log(torch.tensor(1e-3)))
    return dict(
        x_proj_weight=torch.randn(4, R + 2 * N, D, generator=g) * D ** -0.5,
        dt_projs_weight=torch.randn(4, D, R, generator=g) * R ** -0.5,
        dt_projs_bias=dt + torch.log(-torch.expm1(-dt)),
        A_logs=torch.log(torch.arange(1, N + 1).float())[None].repeat(4 * D, 1) + 0.05 * torch.randn(4 * D, N, generator=g),
        Ds=1 + 0.1 * torch.randn(4 * D, generator=g))


def _x(B, D, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, D, H, W, generator=g), torch.randn(B, H, W, D, generator=g)


def _inputs(b, KD, K, N, L, seed, device="cpu"):
    g = torch.Generator().manual_seed(seed)
    u = torch.randn(b, KD, L, generator=g) * 0.5
    delta = torch.randn(b, KD, L, generator=g) * 0.5 - 2
    A = -torch.exp(torch.log(torch.arange(1, N + 1).float())[None].repeat(KD, 1) + 0.1 * torch.randn(KD, N, generator=g))
    Bm, Cm = torch.randn(b, K, N, L, generator=g), torch.randn(b, K, N, L, generator=g)
    D = 1 + 0.1 * torch.randn(KD, generator=g)
    bias = torch.randn(KD, generator=g) * 0.3
    dout = torch.randn(b, KD, L, generator=g)
    return [t.to(device) for t in (u, delta, A, Bm, Cm, D, bias, dout)]


def cs_inputs(c, B=None, seed=0):
    """(x (B,D,H,W), dy (B,H,W,D), parameters) of a cross-scan case on the CPU in fp32: _params / _x, with every 16th channel's dt
    bias at 23 and its dt_proj row quartered, so that delta + bias stays inside 21 .. 25 there (|delta| < 2: the row's product
    with the x_dbl rows has a standard deviation of a quarter) and the v > 20 branch is taken on 1/16 of the rows"""
    B = c.B if B is None else B
    p = _params(c.D, c.N, c.R, seed=c.D + c.N + c.R + seed)
    p["dt_projs_bias"][:, ::HOT_EVERY] = HOT_BIAS
    p["dt_projs_weight"][:, ::HOT_EVERY] *= 0.25
    p["A"] = -torch.exp(p["A_logs"])            # the fp32 A the kernels are handed; the references take their A from it
    x, dy = _x(B, c.D, c.H, c.W, seed=c.D * c.N + c.H * c.W + seed)
    return x, dy, p


def sb_inputs(c):
    """(u, delta, A, B, C, D, delta_bias, dout) of a reference-layout case on the CPU in fp32 (D / delta_bias None where the case
    has none): _inputs; with softplus, every 16th channel's delta is clamped to -3.5 .. -0.5 and meets a bias of 25 (added to
    delta itself where there is no delta_bias): delta + bias in 21.5 .. 24.5.  Without softplus: delta = 0.1 |delta|, as
    test_gpu_scan_bwd.py draws it, and the bias likewise."""
    u, delta, A, Bm, Cm, D, bias, dout = _inputs(c.batch, c.KD, c.K, c.N, c.L, seed=c.KD + c.N + c.L)
    if c.softplus:
        delta[:, ::HOT_EVERY] = delta[:, ::HOT_EVERY].clamp(-3.5, -0.5)
        if c.has_bias:
            bias[::HOT_EVERY] = 25.0
        else:
            delta[:, ::HOT_EVERY] += 25.0
    else:
        delta, bias = delta.abs() * 0.1, bias.abs() * 0.1          # dt = delta + bias itself: kept >= 0, or exp(dt A) grows without bound
    return [u, delta, A, Bm, Cm, D if c.has_D else None, bias if c.has_bias else None, dout]


# ---- the fp64 restatement of the cross-scan ----------------------------------------------------------------------------------
def _scan_f64_fwd(u, delta, A, B, C, D, bias):
    """y of the selective scan (softplus), in u's dtype (float64 for the reference), by a loop over the sequence on u's device"""
    b, KD, L = u.shape
    K, N = B.shape[1], A.shape[1]
    dt = F.softplus(delta + bias[None, :, None])
    Bx, Cx = B.repeat_interleave(KD // K, dim=1), C.repeat_interleave(KD // K, dim=1)      # (b, KD, N, L)
    y = torch.empty_like(u)
    h = torch.zeros(b, KD, N, dtype=u.dtype, device=u.device)
    for c0 in range(0, L, 1024):
        c1 = min(c0 + 1024, L)
        a = torch.exp(dt[:, :, c0:c1, None] * A[None, :, None])
        bu = (dt[:, :, c0:c1] * u[:, :, c0:c1])[..., None] * Bx[..., c0:c1].transpose(2, 3)
        cc = Cx[..., c0:c1].transpose(2, 3)
        for i in range(c1 - c0):
            h = a[:, :, i] * h + bu[:, :, i]
            y[:, :, c0 + i] = (h * cc[:, :, i]).sum(-1)
    return y + D[None, :, None] * u


class _ScanF64(torch.autograd.Function):
    """the scan with scan_bwd_ref's hand-written gradients, in the dtype of its inputs: float64 is the reference, float32 the
    same restatement in the kernels' precision"""

    @staticmethod
    def forward(ctx, u, delta, A, B, C, D, bias):
        ctx.save_for_backward(u, delta, A, B, C, D, bias)
        return _scan_f64_fwd(u, delta, A, B, C, D, bias)

    @staticmethod
    def backward(ctx, dout):
        return scan_grads_f64(*ctx.saved_tensors, dout, True, dtype=dout.dtype)


def _ref_y(x, p, scan):
    """the reference's cross_selective_scan up to out_norm: (B, H, W, D)"""
    from oracle import nets
    Bn, D, H, W = x.shape
    N = p["A_logs"].shape[1]
    K, _, R = p["dt_projs_weight"].shape
    xs = nets.efficient_scan(x)
    L = xs.shape[-1]
    x_dbl = torch.einsum("bkdl,kcd->bkcl", xs, p["x_proj_weight"])
    dts, Bs, Cs = torch.split(x_dbl, [R, N, N], dim=2)
    dts = torch.einsum("bkrl,kdr->bkdl", dts, p["dt_projs_weight"])
    ys = scan(xs.reshape(Bn, -1, L), dts.reshape(Bn, -1, L), -torch.exp(p["A_logs"]), Bs.contiguous(), Cs.contiguous(),
              p["Ds"], p["dt_projs_bias"].reshape(-1))
    y = nets.efficient_merge(ys.view(Bn, K, -1, L), H, W)
    return y.transpose(1, 2).reshape(Bn, H, W, D)


def cs_xdbl_rows(x, p):
    """the x_proj rows as the kernels store them, [4, B, L, R + 2N] at row h2 * W2 + w2 whatever the direction, and
    v = delta + bias (B, 4, D, L) in scan order; in x's dtype"""
    from oracle import nets
    Bn, D, H, W = x.shape
    H2, W2 = (H + 1) // 2, (W + 1) // 2
    xs = nets.efficient_scan(x)
    xd = torch.einsum("bkdl,kcd->bklc", xs, p["x_proj_weight"])
    CD = xd.shape[-1]
    R = p["dt_projs_weight"].shape[2]
    v = torch.einsum("bklr,kdr->bkdl", xd[..., :R], p["dt_projs_weight"]) + p["dt_projs_bias"].reshape(1, 4, D, 1)
    col = lambda t: t.reshape(Bn, W2, H2, CD).transpose(1, 2).reshape(Bn, H2 * W2, CD)
    return torch.stack([xd[:, 0], col(xd[:, 1]), xd[:, 2], col(xd[:, 3])], 0), v


CS_PARAMS = ("x_proj_weight", "dt_projs_weight", "dt_projs_bias", "A_logs", "Ds")
CS_OUTPUTS = ("y", "x_dbl", "dx", "dx_proj_w", "ddtw", "ddtb", "dA", "dDs")
CS_POSITION = ("y", "x_dbl", "dx")                                   # per-position outputs: the 1e-5 gate; the others 1e-4


def cs_reference(x, dy, p, device, dtype):
    """the outputs of the forward + backward calls (CS_OUTPUTS, as the C ABI hands them out: dx NCHW, dA the gradient of
    A = p["A"], the fp32 values the kernels read), restated with torch in `dtype` on `device`"""
    xx = x.to(device, dtype).requires_grad_()
    pp = {k: p[k].to(device, dtype) for k in CS_PARAMS}
    pp["A_logs"] = torch.log(-p["A"].to(device, dtype))
    pp = {k: v.requires_grad_() for k, v in pp.items()}
    y = _ref_y(xx, pp, _ScanF64.apply)
    g = torch.autograd.grad(y, [xx] + [pp[k] for k in CS_PARAMS], dy.to(device, dtype))
    with torch.no_grad():
        rows, _ = cs_xdbl_rows(xx, pp)
        dA = g[4] / -torch.exp(pp["A_logs"])                          # dA_logs = dA * A
    return dict(y=y.detach(), x_dbl=rows, dx=g[0], dx_proj_w=g[1], ddtw=g[2], ddtb=g[3], dA=dA, dDs=g[5])


SB_OUTPUTS = ("du", "ddelta", "dA", "dB", "dC", "dD", "ddelta_bias")
SB_POSITION = ("du", "ddelta", "dB", "dC")

# ---- the gate ----------------------------------------------------------------------------------------------------------------
POSITION_GATE, SUMMED_GATE = 1e-5, 1e-4
MEASURED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scan_bwd_measured_errors.json")
_measured = None
_recorded = {}


def gate4x(key, err, f32_err, blanket):
    """assert err < min(blanket, 4 x the kernel error recorded for `key` on an MI355X, floor 1e-6).  FD_RECORD_SCAN_BWD_ERRORS=<path>
    rewrites <path> with {key: {"kernel": err, "f32": the float32 restatement's error}} instead and holds the blanket gate only."""
    global _measured
    rec = os.environ.get("FD_RECORD_SCAN_BWD_ERRORS")
    if rec:
        _recorded[key] = {"kernel": float(err), "f32": float(f32_err)}
        with open(rec, "w") as f:
            json.dump(dict(sorted(_recorded.items())), f, indent=1)
        assert err < blanket, f"{key}: error {err:.3e} >= gate {blanket:.0e}"
        return
    if _measured is None:
        _measured = json.load(open(MEASURED)) if os.path.exists(MEASURED) else {}
    meas = _measured.get(key, {}).get("kernel")
    lim = blanket if meas is None else min(blanket, max(4.0 * meas, 1e-6))
    assert err < lim, (f"{key}: error {err:.3e} >= gate {lim:.3e}" +
                       (f" (4 x the {meas:.3e} recorded; blanket gate {blanket:.0e})" if meas is not None else ""))
