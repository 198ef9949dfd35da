"""float64 gradients of the selective scan (the op of founddiff_amd.selective_scan_cuda_core.fwd) by a hand-written
forward and reverse loop over the sequence, on whatever device the inputs live on.  Used by tests/test_gpu_scan_bwd.py as
the reference for long sequences, where an autograd graph of every step would be too large.

    dt = softplus(delta + bias) (or without softplus),  a_t = exp(dt_t A),  h_t = a_t h_{t-1} + dt_t B_t u_t
    g_t = dL/dh_t = dout_t C_t + a_{t+1} g_{t+1}
"""
import torch
import torch.nn.functional as F


def scan_grads_f64(u, delta, A, B, C, D, delta_bias, dout, softplus, chunk=1024, dtype=torch.float64):
    """(du, ddelta, dA, dB, dC, dD, ddelta_bias) in float64; B / C 4-D (b, K, N, L); D / delta_bias may be None.
    dtype=torch.float32: the same restatement in the kernels' own precision, for its distance from the float64 one."""
    f = lambda t: None if t is None else t.to(dtype)
    u, delta, A, B, C, D, bias, dout = map(f, (u, delta, A, B, C, D, delta_bias, dout))
    b, KD, L = u.shape
    K, N = B.shape[1], A.shape[1]
    Dg = KD // K
    v = delta + (bias[None, :, None] if bias is not None else 0)
    if softplus:
        dt = F.softplus(v)
        dfac = torch.where(v > 20, torch.ones_like(v), torch.sigmoid(v))
    else:
        dt, dfac = v, torch.ones_like(v)
    # (b, K, Dg, L, 1) per channel, (b, K, 1, L, N) per group, (K, Dg, 1, N) per state
    u5, dt5, dy5 = (t.reshape(b, K, Dg, L, 1) for t in (u, dt, dout))
    B5, C5 = (t.permute(0, 1, 3, 2).unsqueeze(2) for t in (B, C))
    A4 = A.reshape(K, Dg, 1, N)
    H = torch.empty(b, K, Dg, L, N, dtype=dtype, device=u.device)
    G = torch.empty_like(H)
    spans = [(c0, min(c0 + chunk, L)) for c0 in range(0, L, chunk)]
    h = torch.zeros(b, K, Dg, N, dtype=dtype, device=u.device)
    for c0, c1 in spans:
        a = torch.exp(dt5[:, :, :, c0:c1] * A4)
        bu = dt5[:, :, :, c0:c1] * B5[:, :, :, c0:c1] * u5[:, :, :, c0:c1]
        for i in range(c1 - c0):
            h = a[:, :, :, i] * h + bu[:, :, :, i]
            H[:, :, :, c0 + i] = h
    x = torch.zeros_like(h)                 # a_{t+1} g_{t+1}
    for c0, c1 in reversed(spans):
        a = torch.exp(dt5[:, :, :, c0:c1] * A4)
        c = dy5[:, :, :, c0:c1] * C5[:, :, :, c0:c1]
        for i in reversed(range(c1 - c0)):
            g = c[:, :, :, i] + x
            G[:, :, :, c0 + i] = g
            x = a[:, :, :, i] * g
    du = torch.empty(b, K, Dg, L, dtype=dtype, device=u.device)
    ddt = torch.empty_like(du)
    dB = torch.empty(b, K, L, N, dtype=dtype, device=u.device)
    dC = torch.empty_like(dB)
    dA = torch.zeros(K, Dg, N, dtype=dtype, device=u.device)
    for c0, c1 in spans:
        s = slice(c0, c1)
        Hc, Gc = H[:, :, :, s], G[:, :, :, s]
        Hp = torch.cat([torch.zeros_like(Hc[:, :, :, :1]), Hc[:, :, :, :-1]], 3) if c0 == 0 else H[:, :, :, c0 - 1:c1 - 1]
        a = torch.exp(dt5[:, :, :, s] * A4)
        gdt = Gc * dt5[:, :, :, s]
        w = Gc * a * Hp
        dC[:, :, s] = (dy5[:, :, :, s] * Hc).sum(2)
        dB[:, :, s] = (gdt * u5[:, :, :, s]).sum(2)
        du[:, :, :, s] = (gdt * B5[:, :, :, s]).sum(-1)
        ddt[:, :, :, s] = (Gc * B5[:, :, :, s] * u5[:, :, :, s] + A4 * w).sum(-1)
        dA += (dt5[:, :, :, s] * w).sum((0, 3))
    du = du.reshape(b, KD, L)
    if D is not None:
        du = du + D[None, :, None] * dout
    ddelta = ddt.reshape(b, KD, L) * dfac
    dD = (dout * u).sum((0, 2)) if D is not None else None
    dbias = ddelta.sum((0, 2)) if bias is not None else None
    return du, ddelta, dA.reshape(KD, N), dB.permute(0, 1, 3, 2), dC.permute(0, 1, 3, 2), dD, dbias
