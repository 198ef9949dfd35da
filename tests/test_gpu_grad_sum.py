"""csrc/fd_grad_sum.hip on the GPU: fd_grads_pack_f32 and fd_grads_rank_sum_f32 over ClipAdamEMA's tables, through
diffusion_train.GradReducer's pack() and rank_sum() with the rows of the other ranks written into its receive buffer by hand.
Expected: acc = zeros; acc = acc + G[m] for m in global order (m = a W + r), by torch in fp32 -- equality is bitwise.  The inputs mix
magnitudes so that the order of addition decides the result; the test asserts that of its own inputs first, on the CPU."""
import datetime
import os
import socket

import pytest
import torch

pytestmark = pytest.mark.gpu
NUMELS = (1, 3, 4, 4095, 4096, 4097, 8193)
NONE_AT = 3                               # the tensor whose .grad is None, in the middle of the list
MISALIGNED_AT = 5                         # the tensor whose gradient sits at a 4-byte-misaligned address


@pytest.fixture(scope="module")
def group():
    """a process group of one rank (gloo): GradReducer asks an initialised group for W; the rows of the other ranks are written
    into its receive buffer by the tests"""
    import torch.distributed as dist
    assert not dist.is_initialized()
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1,
                            timeout=datetime.timedelta(seconds=120))
    yield dist.group.WORLD
    dist.destroy_process_group()


def _mixed(gen, M, n):
    """(M, n): per element one term near +1e8 and (from two terms on) its exact negative, in two slots drawn per element, and terms
    of magnitudes 1e-3 .. 4e5 in the others: whether a small term survives depends on whether it is added before, between or
    after the two large ones"""
    mags = torch.tensor([1.0, -1.0, 1e-3, 3e4, -7e2, 4e5, 60.0, -9e3])
    v = mags[torch.randint(0, len(mags), (M, n), generator=gen)] * (0.5 + torch.rand(M, n, generator=gen))
    big = 1e8 * (0.5 + torch.rand(1, n, generator=gen))
    slots = torch.rand(M, n, generator=gen).argsort(0)
    v.scatter_(0, slots[0:1], big)
    if M >= 2:
        v.scatter_(0, slots[1:2], -big)
    return v


def _inputs(W, rounds, seed):
    """G[m][i]: the gradient of tensor i in global micro-batch m, on the CPU"""
    gen = torch.Generator().manual_seed(seed)
    per_tensor = [_mixed(gen, W * rounds, n) for n in NUMELS]
    return [[v[m].clone() for v in per_tensor] for m in range(W * rounds)]


def _expected(G, order=None):
    out = []
    for i, n in enumerate(NUMELS):
        acc = torch.zeros(n)
        for m in (order or range(len(G))):
            acc = acc + G[m][i]
        out.append(acc)
    return out


def _params():
    ps = [torch.zeros(n, device="cuda", requires_grad=True) for n in NUMELS]
    return ps


def _set_grads(ps, grads):
    """the gradients of one micro-batch; NONE_AT has none, MISALIGNED_AT's is a view one float into a larger buffer"""
    keep = []
    for i, (p, g) in enumerate(zip(ps, grads)):
        if i == NONE_AT:
            p.grad = None
        elif i == MISALIGNED_AT:
            buf = torch.full((p.numel() + 9,), 7.0, device="cuda")
            view = buf[1:1 + p.numel()]
            view.copy_(g)
            assert view.data_ptr() % 16 == 4
            p.grad = view
            keep.append(buf)
        else:
            p.grad = g.cuda().clone()
    return keep


@pytest.mark.parametrize("rounds", [1, 3])
@pytest.mark.parametrize("W", [1, 2, 3, 8])
def test_pack_and_rank_sum(group, W, rounds):
    from founddiff_amd import diffusion_train as dt
    G = _inputs(W, rounds, seed=10 * W + rounds)
    want = _expected(G)
    if W >= 2 and W * rounds >= 3:        # (one rank has no order; two terms give one sum either way: float addition commutes)
        rev = _expected(G, [a * W + r for a in range(rounds) for r in reversed(range(W))])
        live = [i for i in range(len(NUMELS)) if i != NONE_AT]
        changed = sum(int((rev[i] != want[i]).sum()) for i in live) / sum(NUMELS[i] for i in live)
        print(f"[measured] W={W} rounds={rounds}: reversing the rank order changes {changed:.2%} of the elements")
        assert changed >= 0.25
    ps = _params()
    opt = dt.ClipAdamEMA(ps, None)
    red = dt.GradReducer(opt, group)
    assert red.world == 1 and red.tail == 4 and red.P == sum((n + 3) & ~3 for n in NUMELS) and red.N == red.P + 4
    red.world, red.recv = W, torch.full((W, red.N), float("nan"), device="cuda")      # the other ranks' rows are made here
    offs = [0]
    for n in NUMELS:
        offs.append(offs[-1] + ((n + 3) & ~3))
    rank = W - 1                          # this process plays the last rank: its row is packed by the kernel
    for a in range(rounds):
        m = a * W + rank
        keep = _set_grads(ps, G[m])
        red.flat.fill_(float("nan"))
        losses = [torch.tensor(float(m + 1), device="cuda"), torch.tensor(0.25 * (m + 1), device="cuda")]
        flat = red.pack(losses, zero=True).clone()
        # the packed row: gradients at their offsets, zeros in the padding and for the tensor without a gradient, the tail
        for i, n in enumerate(NUMELS):
            seg = flat[offs[i]:offs[i + 1]].cpu()
            src = torch.zeros(n) if i == NONE_AT else G[m][i]
            assert torch.equal(seg[:n], src), (i, n)
            assert torch.equal(seg[n:], torch.zeros(offs[i + 1] - offs[i] - n)), (i, n)
        assert flat[red.P:].cpu().tolist() == [float(m + 1), 0.25 * (m + 1), 0.0, 0.0]
        # the sources are zeroed, nothing around the misaligned one is written, the None tensor stays None
        for i, p in enumerate(ps):
            if i == NONE_AT:
                assert p.grad is None
            else:
                assert not bool(p.grad.any()), i
        buf = keep[0].cpu()
        assert float(buf[0]) == 7.0 and bool((buf[1 + NUMELS[MISALIGNED_AT]:] == 7.0).all())
        # the rows of the round, this rank's from the kernel
        for r in range(W):
            if r == rank:
                red.recv[r].copy_(flat)
                continue
            row = torch.zeros(red.N)
            for i, n in enumerate(NUMELS):
                if i != NONE_AT:
                    row[offs[i]:offs[i] + n] = G[a * W + r][i]
            row[red.P], row[red.P + 1] = float(a * W + r + 1), 0.25 * (a * W + r + 1)
            red.recv[r].copy_(row)
        red.rank_sum(first=a == 0, last=a == rounds - 1)
    for i, p in enumerate(ps):
        if i == NONE_AT:
            assert p.grad is None
            continue
        assert torch.equal(p.grad.cpu(), want[i]), (i, NUMELS[i], W, rounds)
    buf = keep[0].cpu()
    assert float(buf[0]) == 7.0 and bool((buf[1 + NUMELS[MISALIGNED_AT]:] == 7.0).all())       # the scalar path stays in bounds
    # the losses: summed in the same order, float32
    l0, l1 = torch.zeros(()), torch.zeros(())
    for m in range(W * rounds):
        l0, l1 = l0 + torch.tensor(float(m + 1)), l1 + torch.tensor(0.25 * (m + 1))
    got = red.losses()
    assert len(got) == 2 and got[0].shape == () and torch.equal(got[0].cpu(), l0) and torch.equal(got[1].cpu(), l1)


def test_aligned_and_scalar_paths_agree(group):
    """the same values through the 16-byte path and, at a misaligned address, through the scalar path: the same bits"""
    from founddiff_amd import diffusion_train as dt
    gen = torch.Generator().manual_seed(3)
    n, W = 4097, 3
    rows = list(_mixed(gen, W, n))
    out = []
    for shift in (0, 1):
        p = torch.zeros(n, device="cuda", requires_grad=True)
        buf = torch.zeros(n + 8, device="cuda")
        p.grad = buf[shift:shift + n]
        opt = dt.ClipAdamEMA([p], None)
        red = dt.GradReducer(opt, group)
        red.world, red.recv = W, torch.zeros(W, red.N, device="cuda")
        for r in range(W):
            red.recv[r, :n].copy_(rows[r])
        opt._upload_table()
        red.rank_sum(True, True)
        out.append(p.grad.cpu().clone())
    want = torch.zeros(n)
    for r in range(W):
        want = want + rows[r]
    assert torch.equal(out[0], want) and torch.equal(out[1], want)


def test_arguments(group):
    from founddiff_amd import _lib as L, diffusion_train as dt
    from founddiff_amd._train import ptr, stream
    p = torch.zeros(8, device="cuda", requires_grad=True)
    p.grad = torch.ones(8, device="cuda")
    opt = dt.ClipAdamEMA([p], None)
    red = dt.GradReducer(opt, group)
    with pytest.raises(RuntimeError, match="tail holds 4"):
        red.pack([torch.zeros((), device="cuda")] * 5)
    opt._upload_table()
    dev = p.device
    with pytest.raises(L.FoundDiffHipError, match="W must be in"):
        L.call("fd_grads_rank_sum_f32", ptr(opt._chunks), ptr(opt._table), ptr(red._offs), opt.nchunk, ptr(red.recv), 65, red.N,
               ptr(red.acc), red.P, 1, 1, stream(dev))
    with pytest.raises(L.FoundDiffHipError, match="N = P"):
        L.call("fd_grads_rank_sum_f32", ptr(opt._chunks), ptr(opt._table), ptr(red._offs), opt.nchunk, ptr(red.recv), 1, red.N + 4,
               ptr(red.acc), red.P, 1, 1, stream(dev))
    with pytest.raises(L.FoundDiffHipError, match="null pointer"):
        L.call("fd_grads_pack_f32", ptr(opt._chunks), ptr(opt._table), ptr(red._offs), opt.nchunk, None, red.P, None, 0, 1, stream(dev))
    assert bool((p.grad == 1).all())      # a refused call writes nothing
