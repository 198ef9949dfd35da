"""Sampling the two-U-Net and pred_noise models on the captured-loop path: fd_obj_begin / fd_res_step_obj_keyed at the C ABI against
a float64 evaluation of the header's formulas, and ResidualDiffusion's loops of every plan -- graph equals eager equals the eager
_generic_loop, a slice a function of its input and seed alone (streams, batch, group split, ensembles, tiles), graphs forgotten
with the weights.  The tiny model of the variant tests (dim 32, mults (1, 2), TINY_CLIP, 64 x 64, synthetic weights, fp32)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
TINY_CLIP = dict(layers=(2, 1, 1, 1), width=16, embed_dim=1024)
PLANS = {   # name -> (num_unet, objective, test_res_or_noise); tests/test_gpu_e2e.py VARIANTS without the 3-plane models
    "pred_noise": (1, "pred_noise", "noise"), "res_noise": (2, "pred_res_noise", "res_noise"),
    "rn_noise": (2, "pred_res_noise", "noise"), "rn_res": (2, "pred_res_noise", "res"), "x0_noise": (2, "pred_x0_noise", "res_noise"),
}
U = 2.0 ** -24
T = 1000


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


# ---- 1. the kernels alone
@functools.lru_cache(maxsize=None)
def _table():
    """(T, 8) rows {ac, bc, omac, c1, c2, c3, logvar, 0} of the schedule sampling runs under"""
    from founddiff_amd.DADiff import residual_schedule
    s = residual_schedule(T, after_init=True)
    cols = [s[k] for k in ("alphas_cumsum", "betas_cumsum", "one_minus_alphas_cumsum", "posterior_mean_coef1", "posterior_mean_coef2",
                           "posterior_mean_coef3", "posterior_log_variance_clipped")]
    return torch.stack(cols + [torch.zeros(T)], 1).contiguous()


SEEDS = [7, 2 ** 40 + 12345, 2 ** 62 - 1]


def _inputs(B, npix, seed):
    g = torch.Generator().manual_seed(seed)
    o0, o1 = torch.randn(B, npix, generator=g), torch.randn(B, npix, generator=g)
    xt = torch.randn(B, npix, generator=g) * 0.6
    xin = torch.rand(B, npix, generator=g) * 2 - 1
    return [v.cuda() for v in (o0, o1, xt, xin)]


def _keyed(seeds, t, B, npix):
    from founddiff_amd import _lib as L
    z = torch.empty(B, npix, device="cuda")
    L.call("fd_keyed_normal", seeds.data_ptr(), int(t), z.data_ptr(), B, npix, _stream())
    return z


def _step(mode, o0, o1, xt, xin, t, seeds, out=None, table=None):
    """fd_res_step_obj_keyed with the counter at t; out=None: in place on a copy of xt"""
    from founddiff_amd import _lib as L
    B, npix = xt.shape
    tab = (_table() if table is None else table).cuda()
    t_dev = torch.tensor([t], dtype=torch.int32, device="cuda")
    if out is None:
        out = xt.clone()
        src = out
    else:
        src = xt
    L.call("fd_res_step_obj_keyed", mode, _p(o0 if mode != 1 else None), _p(o1 if mode != 0 else None), src.data_ptr(), xin.data_ptr(),
           tab.data_ptr(), t_dev.data_ptr(), seeds.data_ptr(), out.data_ptr(), B, npix, T, _stream())
    torch.cuda.synchronize()
    assert int(t_dev) == t                                                        # the step kernel only reads the counter
    return out


def _ref64(mode, o0, o1, x, xi, row, z, t):
    """(value, first-order rounding bound) of the header's formulas in float64; see test_step_kernel_vs_float64"""
    a, bb, oma, c1, c2, c3, lv = [float(v) for v in row[:7]]
    clamp = lambda v: np.clip(v, -1.0, 1.0)
    e_pr = e_xs = 0.0
    if mode == 0:
        pr = clamp(o0)
        d = xi - pr
        xs, e_xs = clamp(d), U * np.abs(d)
    elif mode in (1, 2):
        y = xi if mode == 1 else clamp(o0)
        p1 = a * y
        r1 = x - p1
        p2 = bb * o1
        n = r1 - p2
        e_n = U * (np.abs(p1) + np.abs(r1) + np.abs(p2) + np.abs(n))
        if mode == 1:
            q = n / oma
            xs, e_xs = clamp(q), e_n / abs(oma) + U * np.abs(q)
            d = xi - xs
            pr, e_pr = clamp(d), e_xs + U * np.abs(d)
        else:
            pr, xs, e_xs = y, clamp(n), e_n
    else:
        d = xi - o0
        pr, e_pr = clamp(d), U * np.abs(d)
        xs = clamp(o0)
    sd = float(np.exp(0.5 * lv)) if t > 0 else 0.0
    terms = [c1 * x, c2 * pr, c3 * xs, sd * z]
    mag = sum(np.abs(v) for v in terms)
    bound = abs(c2) * e_pr + abs(c3) * e_xs + U * mag + 4 * U * np.abs(terms[3]) + 3 * U * mag
    return sum(terms), bound * (1 + 2.0 ** -10)


@pytest.mark.parametrize("npix", [37 * 41, 64 * 64])
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_step_kernel_vs_float64(mode, npix):
    """fd_res_step_obj_keyed, B = 3, the counter at t in {0, 1, 17, 999}, rows of residual_schedule(1000, after_init=True), in place
    and out of place, against float64 on the noise fd_keyed_normal gives for (seeds, t).

    The gate, first order in u = 2^-24, every fp32 operation contributing u |its result| (a fused multiply-add only drops a
    rounding); the inputs and the table row are exact, clamp is 1-Lipschitz and exact on an exact argument:
      mode 0: pr = clamp(o0) exact;  xs = clamp(xi - pr): u |xi - pr|
      mode 1: n = x - a xi - bb o1, four operations: e_n = u (|a xi| + |x - a xi| + |bb o1| + |n|);  q = n / omac, a correctly
              rounded division: e_n / |omac| + u |q|;  xs = clamp(q) the same;  pr = clamp(xi - xs): e_xs + u |xi - xs|
      mode 2: pr = clamp(o0) exact;  xs = clamp(x - a pr - bb o1): e_n with pr in xi's place
      mode 3: pr = clamp(xi - o0): u |xi - o0|;  xs = clamp(o0) exact
      out = c1 x + c2 pr + c3 xs + sd z:  |c2| e_pr + |c3| e_xs, u per product (u M, M = |c1 x| + |c2 pr| + |c3 xs| + |sd z|), 4 u
            |sd z| for sd = expf(logvar / 2) within 2 ulp (the halving is exact), and u times a partial sum of at most M for each of
            the three additions: 3 u M.
    The bound is taken per pixel, times 1 + 2^-10 for the second-order terms.  Observed on the MI355X: DESIGN.md section 4."""
    B = 3
    o0, o1, xt, xin = _inputs(B, npix, 100 + mode)
    seeds = torch.tensor(SEEDS, dtype=torch.int64).cuda()
    tab = _table()
    worst = 0.0
    for t in (0, 1, 17, 999):
        out = torch.full((B, npix), float("nan"), device="cuda")
        _step(mode, o0, o1, xt, xin, t, seeds, out=out)
        assert torch.equal(_step(mode, o0, o1, xt, xin, t, seeds), out), t                     # in place: the same bits
        z = _keyed(seeds, t, B, npix)
        f64 = lambda v: v.double().cpu().numpy()
        want, bound = _ref64(mode, f64(o0), f64(o1), f64(xt), f64(xin), tab[t].double().numpy(), f64(z), t)
        err = np.abs(f64(out) - want)
        ratio = float((err / np.maximum(bound, 1e-300)).max())
        print(f"[measured] fd_res_step_obj_keyed mode {mode} npix {npix} t {t}: max |err| {err.max():.3e}, max err / bound {ratio:.3f}")
        worst = max(worst, ratio)
        assert np.isfinite(f64(out)).all() and bool((err <= bound).all()), (t, float(err.max()), ratio)
        other = torch.tensor([s + 1 for s in SEEDS], dtype=torch.int64).cuda()
        if t == 0:                                                                               # no noise at t = 0
            assert torch.equal(_step(mode, o0, o1, xt, xin, 0, other), out)
        else:
            assert not torch.equal(_step(mode, o0, o1, xt, xin, t, other), out)
        # slice b is a function of its own row and seed: alone (B = 1) it has the bits it has in the batch of 3
        for b in (1, 2):
            one = _step(mode, o0[b:b + 1].contiguous(), o1[b:b + 1].contiguous(), xt[b:b + 1].contiguous(), xin[b:b + 1].contiguous(),
                        t, seeds[b:b + 1].contiguous())
            assert torch.equal(one[0], out[b]), (t, b)
    assert worst <= 1.0


def test_step_kernel_scalar_path_has_the_same_bits():
    """pointers one float past a 16-byte boundary take the one-pixel-at-a-time form of the kernel"""
    B, npix = 3, 64 * 64
    seeds = torch.tensor(SEEDS, dtype=torch.int64).cuda()

    def off(v):
        buf = torch.empty(v.numel() + 4, device="cuda")
        w = buf[1:1 + v.numel()].view(v.shape)
        w.copy_(v)
        assert w.data_ptr() % 16 == 4
        return w
    for mode in range(4):
        o0, o1, xt, xin = _inputs(B, npix, 200 + mode)
        want = _step(mode, o0, o1, xt, xin, 17, seeds)
        got = _step(mode, off(o0), off(o1), off(xt), off(xin), 17, seeds, out=off(torch.zeros(B, npix, device="cuda")))
        assert torch.equal(got, want), mode


def test_obj_begin():
    from founddiff_amd import _lib as L
    times0 = torch.arange(T, dtype=torch.float32).cuda() * 0.5
    times1 = torch.arange(T, dtype=torch.float32).cuda() * 0.25 + 3
    B = 3

    def begin(t, use0=True, use1=True):
        t_dev = torch.tensor([t], dtype=torch.int32, device="cuda")
        b0, b1 = torch.full((B + 2,), -7.0, device="cuda"), torch.full((B + 2,), -7.0, device="cuda")
        L.call("fd_obj_begin", t_dev.data_ptr(), _p(times0 if use0 else None), _p(times1 if use1 else None), _p(b0 if use0 else None),
               _p(b1 if use1 else None), B, T, _stream())
        torch.cuda.synchronize()
        return int(t_dev), b0.cpu().tolist(), b1.cpu().tolist()
    assert begin(T) == (T - 1, [499.5] * 3 + [-7.0] * 2, [252.75] * 3 + [-7.0] * 2)              # T -> T - 1, B entries and no more
    assert begin(18) == (17, [8.5] * 3 + [-7.0] * 2, [7.25] * 3 + [-7.0] * 2)
    assert begin(1)[0] == 0 and begin(0) == (0, [0.0] * 3 + [-7.0] * 2, [3.0] * 3 + [-7.0] * 2)  # clamps at 0
    assert begin(18, use1=False) == (17, [8.5] * 3 + [-7.0] * 2, [-7.0] * 5)                      # a NULL buffer: the other alone
    assert begin(18, use0=False) == (17, [-7.0] * 5, [7.25] * 3 + [-7.0] * 2)


# ---- the loops
@functools.lru_cache(maxsize=None)
def _weights(nu):
    from founddiff_amd import arch, synth
    w = {}
    for i in range(nu):
        w.update(synth.synth_state_dict(arch.da_unet_spec(32, (1, 2), prefix=f"model.unet{i}.", clip=TINY_CLIP), seed=i))
    return w


def _model(name, S):
    from founddiff_amd.DADiff import ResidualDiffusion, UnetRes, load_weights
    nu, obj, tst = PLANS[name]
    net = UnetRes(dim=32, dim_mults=(1, 2), num_unet=nu, condition=True, objective=obj, test_res_or_noise=tst, precision="fp32",
                  clip_cfg=TINY_CLIP)
    dif = ResidualDiffusion(net, image_size=64, timesteps=T, sampling_timesteps=S, objective=obj, loss_type="l2", condition=True,
                            sum_scale=0.01, test_res_or_noise=tst)
    load_weights(dif, _weights(nu))
    dif = dif.to("cuda")
    dif.init()
    return dif


@functools.lru_cache(maxsize=None)
def _slices(n):
    from founddiff_amd import synth
    return torch.from_numpy(synth.ct_phantom(n, 64, seed=10)[1]).cuda()


def _kinds(dif):
    return set(dif._engines()[0].graphs)


@pytest.mark.parametrize("name", sorted(PLANS))
def test_graph_equals_eager(name):
    """4-step DDIM and the ancestral sampler bounded to one chunk (50 steps): use_graph=True has the bits of use_graph=False, the
    plan's first engine owns the loop's graph, and the DDIM image is the last image of the eager _generic_loop (last=False under
    the same x_T).  'rn_res' is the shipped plan (0, True, False, 0) on a two-U-Net model: its loops are ddim_sample's own and
    _ancestral_keyed, kinds "ddim_loop" / "anc", whose eager ancestral form has no bounded run -- DDIM only."""
    shipped = name == "rn_res"
    x, seeds = _slices(2), [5, 2 ** 41 + 3]
    dif = _model(name, 4)
    assert dif._is_shipped() == shipped
    g = dif.sample([x], batch_size=2, slice_seeds=seeds)
    assert _kinds(dif) == ({"ddim_loop"} if shipped else {"obj_ddim"})
    dif.use_graph = False
    e = dif.sample([x], batch_size=2, slice_seeds=seeds)
    assert torch.equal(g[0], e[0]) and torch.equal(g[-1], e[-1]) and bool(torch.isfinite(g[-1]).all())
    nz = dif._keyed_noise(torch.tensor(seeds, dtype=torch.int64).cuda(), dif.X_T_STEP, (2, 1, 64, 64))
    traj = dif.sample([x], batch_size=2, last=False, noise=nz)
    assert len(traj) == 5 and torch.equal(traj[-1], g[-1]) and torch.equal(traj[0], g[0])
    if shipped:
        return
    dif = _model(name, T)
    dif._anc_max_chunks = 1
    g = dif.sample([x], batch_size=2, slice_seeds=seeds)
    assert _kinds(dif) == {"obj_anc"} and dif._anc_steps_run == 50
    dif.use_graph = False
    e = dif.sample([x], batch_size=2, slice_seeds=seeds)
    assert dif._anc_steps_run == 50
    assert torch.equal(g[0], e[0]) and torch.equal(g[-1], e[-1]) and bool(torch.isfinite(g[-1]).all())
    assert not torch.equal(g[-1], g[0])


def test_slice_is_a_function_of_its_input_and_seed():
    """The full 1000 steps of the ancestral sampler on 'res_noise': rows 2:5 of a batch of 8 on two streams are the batch of 3 on one
    stream and the batch of 8 with streams = 1; the same slice under another seed is another image."""
    dif = _model("res_noise", T)
    x = _slices(8).clone()
    x[1] = x[0]
    seeds = [31, 32, 2 ** 40 + 33, 34, 35, 36, 37, 38]
    two = dif.sample([x], batch_size=8, slice_seeds=seeds)
    assert dif._anc_steps_run == T
    assert "obj_anc" in dif.model.unet0.engine(slot=1).graphs and dif.model.unet1.engine(slot=1) is not dif.model.unet1.engine()
    three = dif.sample([x[2:5]], batch_size=3, slice_seeds=seeds[2:5])
    dif.streams = 1
    one = dif.sample([x], batch_size=8, slice_seeds=seeds)
    for j in (0, -1):
        assert torch.equal(two[j][2:5], three[j]) and torch.equal(two[j], one[j]), j
    assert bool(torch.isfinite(two[-1]).all())
    assert not torch.equal(two[-1][0], two[-1][1]) and float((two[-1][0] - two[-1][1]).abs().max()) > 1e-4


def test_group_split_and_workspace():
    """16 two-U-Net slices under max_sub_batch = 4 on two streams: groups of 2 x 4 // 2 = 4, each as 2 + 2 -- no engine of either
    U-Net ever holds more than max_sub_batch // 2 = 2 rows -- and the bits of the un-split run (8 + 8)."""
    dif = _model("res_noise", 2)
    x = torch.cat([_slices(8), _slices(8).flip(-1)], 0)
    seeds = list(range(50, 66))
    # (x_T given: without it the DDIM sampler keys x_T on the seeds in the group split and draws torch.randn on the streams)
    nz = dif._keyed_noise(torch.tensor(seeds, dtype=torch.int64).cuda(), dif.X_T_STEP, (16, 1, 64, 64))
    dif.streams, dif.max_sub_batch = 2, 4
    cut = dif.sample([x], batch_size=16, noise=nz, slice_seeds=seeds)
    engines = [e for u in (dif.model.unet0, dif.model.unet1) for e in u._engine.values()]
    assert len(engines) == 4                                                      # two slots of each U-Net
    for e in engines:
        rows = {name: shape for (name, shape, _) in e.buf}
        assert rows["obj_out"][0] == 2 and rows["obj_time"] == (2,) and rows["prompt_emb"][0] == 2 and rows["obj_ddim_time"] == (2, 2)
        for (name, shape, _) in e.buf:
            if name in ("obj_xin", "obj_img", "obj_out", "prompt_emb", "local_all", "model_out"):
                assert shape[0] <= 2, (name, shape)
            if name == "obj_ddim_par":
                assert shape[1] <= 2, shape
    dif.max_sub_batch = 16
    whole = dif.sample([x], batch_size=16, noise=nz, slice_seeds=seeds)
    assert torch.equal(cut[0], whole[0]) and torch.equal(cut[-1], whole[-1])
    assert max(shape[0] for e in engines for (name, shape, _) in e.buf if name == "obj_out") == 8


def test_ensembles_and_tiles_run_on_the_captured_loop():
    """sample_ensemble (K = 2) and sample_tiled (tile 32, overlap 8) of an ancestral 'res_noise' model, bounded to one chunk: every
    replica and every tile is the batch-1 sample() under its seed, bit for bit, and the loops were captured."""
    from founddiff_amd.ensemble import ensemble_seeds
    from founddiff_amd.tiling import tile_plan, tile_seeds
    dif = _model("res_noise", T)
    dif._anc_max_chunks = 1
    x, seeds = _slices(2), [21, 2 ** 40 + 22]
    ens = dif.sample_ensemble([x], 2, slice_seeds=seeds, return_samples=True)
    assert _kinds(dif) == {"obj_anc"} and dif._anc_steps_run == 50
    rs = ensemble_seeds(np.asarray(seeds, dtype=np.int64), 2)
    for b in range(2):
        for k in range(2):
            one = dif.sample([x[b:b + 1]], batch_size=1, slice_seeds=[int(rs[b, k])])[-1]
            assert torch.equal(ens.samples[b, k], one[0]), (b, k)
    assert not torch.equal(ens.samples[0, 0], ens.samples[0, 1])
    # tiles: the rows _tile_rows hands to the blend
    dif._drop_graphs()
    kept = {}
    rows_of = dif._tile_rows
    dif._tile_rows = lambda *a: kept.setdefault("tiles", rows_of(*a))
    x1 = x[:1]
    out = dif.sample_tiled([x1], 32, 8, slice_seeds=[9])
    del dif._tile_rows
    assert _kinds(dif) == {"obj_anc"} and bool(torch.isfinite(out[1]).all())
    ys = [int(v) for v in tile_plan(64, 32, 8)]
    assert ys == [0, 24, 32] and kept["tiles"].shape == (9, 1, 32, 32)
    ts = tile_seeds(np.asarray([9], dtype=np.int64), 9)
    field = dif._keyed_noise(torch.tensor([9], dtype=torch.int64).cuda(), dif.X_T_STEP, (1, 1, 64, 64))
    for j in range(9):
        win = (slice(None), slice(None), slice(ys[j // 3], ys[j // 3] + 32), slice(ys[j % 3], ys[j % 3] + 32))
        one = dif.sample([x1[win].contiguous()], batch_size=1, noise=field[win].contiguous(), slice_seeds=[int(ts[0, j])])[-1]
        assert torch.equal(kept["tiles"][j], one[0]), j


def test_weights_changed_forgets_the_loops():
    dif = _model("res_noise", 4)
    x, seeds = _slices(2), [1, 2]
    a = dif.sample([x], batch_size=2, slice_seeds=seeds)[-1].clone()
    own = dif._engines()[0]
    assert set(own.graphs) == {"obj_ddim"}
    graph = own.graphs["obj_ddim"][1]
    assert dif.sample([x], batch_size=2, slice_seeds=seeds) is not None and own.graphs["obj_ddim"][1] is graph      # replayed
    dif.weights_changed()
    assert own.graphs == {}
    again = dif._engines()[0]
    assert again is not own and again.graphs == {}
    b = dif.sample([x], batch_size=2, slice_seeds=seeds)[-1]
    assert set(again.graphs) == {"obj_ddim"} and again.graphs["obj_ddim"][1] is not graph
    assert torch.equal(a, b)
    dif.init()
    assert again.graphs == {}
