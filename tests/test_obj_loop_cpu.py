"""The captured-loop path of the plans other than the shipped one, on the CPU: ResidualDiffusion._sample's routing of a two-U-Net
model (recording stubs of tests/sample_routing.py: the concurrent sub-batches, the group split with the halved group, the eager
loop for what the captured loops do not cover, the draws of seeds and x_T), and the step tables of the loops as pure host functions
against the rows _par and _outputs build per step.  Touches no kernel."""
import pytest
import torch

import sample_routing as SR
from founddiff_amd import DADiff

TINY_CLIP = dict(layers=(2, 1, 1, 1), width=16, embed_dim=1024)
PLANS = {   # name -> (num_unet, objective, test_res_or_noise); tests/test_gpu_e2e.py VARIANTS without the 3-plane models
    "pred_noise": (1, "pred_noise", "noise"), "res_noise": (2, "pred_res_noise", "res_noise"),
    "rn_noise": (2, "pred_res_noise", "noise"), "rn_res": (2, "pred_res_noise", "res"), "x0_noise": (2, "pred_x0_noise", "res_noise"),
}
DRAWS = ("randint", "randn", "_keyed_noise")


def _dif(name, S, input_condition=False):
    nu, obj, tst = PLANS[name]
    net = DADiff.UnetRes(dim=32, dim_mults=(1, 2), num_unet=nu, condition=True, objective=obj, test_res_or_noise=tst,
                         clip_cfg=TINY_CLIP, input_condition=input_condition)
    return DADiff.ResidualDiffusion(net, image_size=SR.HW, timesteps=1000, sampling_timesteps=S, objective=obj, loss_type="l2",
                                    condition=True, sum_scale=0.01, test_res_or_noise=tst, input_condition=input_condition)


class TwoRecorder(SR.Recorder):
    """SR.Recorder -- its stubs, its run() -- over a two-U-Net 'pred_res_noise' / 'res_noise' model.  loops=True leaves ddim_sample
    and p_sample_loop real and records the loop they reach instead: _obj_ddim, _obj_ancestral or the eager _generic_loop."""

    def __init__(self, loops=False, input_condition=False):
        self.difs = {S: _dif("res_noise", S, input_condition) for S in SR.AXES["S"]}
        for dif in self.difs.values():
            dif._sample_concurrent = self._sample_concurrent
            dif._keyed_noise = self._keyed_noise
            if loops:
                dif._obj_ddim, dif._obj_ancestral, dif._generic_loop = self._obj_ddim, self._obj_ancestral, self._generic_loop
            else:
                dif.ddim_sample, dif.p_sample_loop = self._ddim_sample, self._p_sample_loop
        self.rows, self.draws = [], 0

    def _obj_ddim(self, x_in, shape, noise, cond=None):
        self.rows.append(["_obj_ddim", list(x_in.shape), list(shape), SR._desc(noise)])
        return self._out(shape)

    def _obj_ancestral(self, x_in, shape, noise, seeds, cond=None):
        self.rows.append(["_obj_ancestral", list(x_in.shape), list(shape), SR._desc(noise), SR._desc(seeds)])
        return self._out(shape)

    def _generic_loop(self, x_in, shape, last, noise, step_noise, ddim, cond=None):
        self.rows.append(["_generic_loop", list(x_in.shape), list(shape), bool(last), SR._desc(noise), step_noise is not None, bool(ddim)])
        return self._out(shape)

    def run3(self, c):
        """run() of a 3-plane model: the same call with x_input = [a, b]"""
        dif = self.difs[c["S"]]
        dif.streams, dif.max_sub_batch = c["streams"], c["msb"]
        shape = (c["B"], 1, SR.HW, SR.HW)
        self.rows, self.draws = [], 0
        saved = DADiff._affine, torch.randint, torch.randn
        DADiff._affine = lambda x, a, b: x * a + b
        torch.randint, torch.randn = self._randint, self._randn
        try:
            dif._sample([torch.full(shape, 0.5), torch.full(shape, 0.25)], c["B"], True, None, None, None)
        finally:
            DADiff._affine, torch.randint, torch.randn = saved
        return self.rows


def _case(**kw):
    c = dict(S=10, B=8, streams=2, msb=16, noise=0, seeds=0, step_noise=0, last=1)
    c.update(kw)
    return c


def test_two_unets_reach_the_streams_and_the_halved_group():
    rec = TwoRecorder()
    assert rec.difs[10]._plan() == (2, True, True, 0) and not rec.difs[10]._is_shipped()
    rec.difs[10].streams, rec.difs[10].max_sub_batch = 2, 16
    assert rec.difs[10]._group_rows() == 16                                     # streams x max_sub_batch // 2
    for S in (10, 1000):
        rows = rec.run(_case(S=S))
        assert [r[0] for r in rows if r[0] not in DRAWS] == ["_sample_concurrent", "returns"], rows
        conc = [r for r in rows if r[0] == "_sample_concurrent"][0]
        assert conc[2] == [8, 1, SR.HW, SR.HW] and conc[4] == 2
        assert (conc[5] is None) == (S == 10)                                   # the ancestral sub-batches carry their seeds
        # below 8 slices: one stream
        assert [r[0] for r in rec.run(_case(S=S, B=2)) if r[0] not in DRAWS] == ["ddim_sample" if S == 10 else "p_sample_loop", "returns"]
        # above streams x max_sub_batch // 2 = 16: consecutive groups of 16, each on the two streams (the shipped plan: 32 + 8)
        rows = rec.run(_case(S=S, B=40))
        assert [r[1][0] for r in rows if r[0] == "_sample_concurrent"] == [16, 16, 8], rows
        assert not [r for r in rows if r[0] in ("ddim_sample", "p_sample_loop")]
        # max_sub_batch = 4: groups of 4 -- and a group of 4 still runs as 2 + 2, so that no engine holds more than 4 // 2 slices
        rows = rec.run(_case(S=S, B=12, msb=4))
        assert [(r[1][0], r[4]) for r in rows if r[0] == "_sample_concurrent"] == [(4, 2)] * 3, rows
        # one stream: groups of max_sub_batch // 2 = 8
        rows = rec.run(_case(S=S, B=40, streams=1))
        assert [r[2][0] for r in rows if r[0] in ("ddim_sample", "p_sample_loop")] == [8] * 5, rows
    assert rec.difs[10]._group_rows() == 8
    rec.difs[10].streams, rec.difs[10].max_sub_batch = 2, 5
    assert rec.difs[10]._group_rows() == 4                                       # kept a multiple of streams
    rec.difs[10].max_sub_batch = 1
    assert rec.difs[10]._group_rows() == 2


def test_draws_are_the_shipped_plans():
    """Every case of the snapshot's axes: a two-U-Net model draws seeds and x_T -- which generator, which shapes, in which order --
    exactly as the shipped plan does with the same group size (max_sub_batch halved), and as the shipped plan's SAME case wherever
    the halved group does not change whether the batch is split."""
    two, one = TwoRecorder(), SR.Recorder()
    draws = lambda rows: [r for r in rows if r[0] in DRAWS]
    same = 0
    for c in SR.CASES:
        got = draws(two.run(c))
        assert got == draws(one.run(dict(c, msb=c["msb"] // 2))), SR.case_id(c)
        full, half = c["streams"] * c["msb"], c["streams"] * c["msb"] // 2
        if (c["B"] > full) == (c["B"] > half):
            assert got == draws(one.run(c)), SR.case_id(c)
            same += 1
    assert same >= len(SR.CASES) // 2


def test_what_stays_on_the_eager_loop():
    rec = TwoRecorder(loops=True)
    loop = lambda rows: [r[0] for r in rows if r[0] not in DRAWS and r[0] != "returns"]
    # covered: the captured loops, on one stream below 8 slices
    assert loop(rec.run(_case(B=2))) == ["_obj_ddim"]
    rows = rec.run(_case(S=1000, B=2, seeds=1))
    assert loop(rows) == ["_obj_ancestral"]
    anc = rows[-2]
    assert anc[4] == [[2], 1000 * SR.GIVEN_SEEDS, 1000 * SR.GIVEN_SEEDS + 1]       # the given seeds reach the loop ...
    assert rows[0][:3] == ["_keyed_noise", anc[4], DADiff.ResidualDiffusion.X_T_STEP]  # ... and key x_T, p_sample_loop's rule
    rows = rec.run(_case(S=1000, B=2))
    assert [r[0] for r in rows] == ["randint", "_keyed_noise", "_obj_ancestral", "returns"]   # seeds: ONE randint on the CPU generator
    # not covered: trajectories, a step_noise callable (ancestral), whatever the batch -- no streams, no split, the eager loop
    for B in (2, 8, 40):
        for S in (10, 1000):
            assert loop(rec.run(_case(S=S, B=B, last=0))) == ["_generic_loop"], (S, B)
        rows = rec.run(_case(S=1000, B=B, step_noise=1))
        assert loop(rows) == ["_generic_loop"] and rows[-2][5] is True, B
    # ... and the 3-plane models
    rec3 = TwoRecorder(loops=True, input_condition=True)
    assert not rec3.difs[10]._captured_plan()
    for B in (2, 8, 40):
        for S in (10, 1000):
            rows = rec3.run3(_case(S=S, B=B))
            assert loop(rows) == ["_generic_loop"] and rows[-1][2] == [B, 1, SR.HW, SR.HW], (S, B)


# ---- the step tables
@pytest.fixture(scope="module", params=sorted(PLANS))
def plan(request):
    dif = _dif(request.param, 4)
    dif.init()                                                                    # the schedule sampling runs under (Trainer.test)
    return request.param, dif


def test_ancestral_table_is_par_row_by_row(plan):
    name, dif = plan
    tab = dif._obj_anc_table()
    assert tab.shape == (1000, 8) and tab.dtype == torch.float32 and tab.is_contiguous()
    hs = dif._hs()
    for t in range(1000):
        k = (float(hs["posterior_mean_coef1"][t]), float(hs["posterior_mean_coef2"][t]), float(hs["posterior_mean_coef3"][t]),
             float(hs["posterior_log_variance_clipped"][t]))                     # p_sample's k
        want = dif._par(torch.full((1,), t, dtype=torch.long), k=k)
        assert torch.equal(tab[t], want[0]), (name, t)


@pytest.mark.parametrize("S,B", [(4, 3), (50, 1)])
def test_ddim_table_is_par_step_by_step(plan, S, B):
    name, dif = plan
    saved = dif.sampling_timesteps
    dif.sampling_timesteps = S
    try:
        par, tt0, tt1 = dif._obj_ddim_table(B)
    finally:
        dif.sampling_timesteps = saved
    assert par.shape == (S, B, 8) and par.dtype == torch.float32 and par.is_contiguous()
    _, r0, r1, tsel0 = dif._plan()
    T = dif.num_timesteps
    times = list(reversed(torch.linspace(-1, T - 1, steps=S + 1).int().tolist()))      # _generic_loop's steps
    acs = dif._hs()["alphas_cumsum"]
    assert len(times) == S + 1 and times[0] == T - 1 and times[-1] == -1
    for i, (time, time_next) in enumerate(zip(times[:-1], times[1:])):
        t_idx = torch.full((B,), time, dtype=torch.long)
        lastf = time_next < 0
        alpha = 0.0 if lastf else float(acs[time] - acs[time_next])
        assert torch.equal(par[i], dif._par(t_idx, k=(alpha, 0., 0., 0.), flag=float(lastf))), (name, i)
        t0 = ((dif.alphas_cumsum if tsel0 == 0 else dif.betas_cumsum)[t_idx] * T).float().contiguous()      # _outputs' time inputs
        t1 = (dif.betas_cumsum[t_idx] * T).float().contiguous()
        assert (tt0 is None) == (not r0) and (tt1 is None) == (not r1)
        assert tt0 is None or torch.equal(tt0[i], t0), (name, i)
        assert tt1 is None or torch.equal(tt1[i], t1), (name, i)
    assert bool(par[-1, :, 7].all()) and not bool(par[:-1, :, 7].any())


def test_time_tables_per_plan(plan):
    name, dif = plan
    t0, t1 = dif._obj_time_tables()
    T = dif.num_timesteps
    ac, bc = (dif.alphas_cumsum * T).float(), (dif.betas_cumsum * T).float()
    want = {"pred_noise": (bc, None), "res_noise": (ac, bc), "rn_noise": (None, bc), "rn_res": (ac, None), "x0_noise": (ac, bc)}[name]
    for got, w in zip((t0, t1), want):
        assert (got is None) == (w is None), name
        if w is not None:
            assert got.shape == (T,) and got.dtype == torch.float32 and torch.equal(got, w), name
    assert not torch.equal(ac, bc)
