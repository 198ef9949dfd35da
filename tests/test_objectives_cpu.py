"""The objective routing rule -- which U-Net runs, at which of the two time inputs, predicting what -- on the CPU; nothing launches.

Part A characterises the rule through the entry points that apply it: ResidualDiffusion._plan / _is_shipped / _group_rows,
UnetRes.forward, diffusion_train.p_losses_fn and ResidualDiffusion.eval_items, against literal tables.  It uses no name of
founddiff_amd/objectives.py: the tables were recorded, and these tests passed, on the tree before that module existed.  Part B pins
the module itself -- the training table and the sampling plan -- to what Part A records, and the module layout around it.
"""
import itertools
import os
import subprocess
import sys

import pytest
import torch

from founddiff_amd import diffusion_train as dt
from founddiff_amd.DADiff import ResidualDiffusion, UnetRes

TINY_CLIP = dict(layers=(2, 1, 1, 1), width=16, embed_dim=1024)
OBJECTIVES = ("pred_res", "pred_noise", "pred_res_noise", "pred_x0_noise")
TESTS = ("None", "res", "noise", "res_noise")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- A1: (num_unet, objective, test_res_or_noise) -> (_plan(), _is_shipped(), _group_rows()) at streams=2, max_sub_batch=16, or
# (where it raises, the exception, a piece of its message)
RAISES = "raises"


def _expected_plan(nu, obj, tst):
    if nu == 1:
        if obj == "pred_res":
            return (0, True, False, 0), True, 32
        if obj == "pred_noise":
            return (1, True, False, 1), False, 32
        return RAISES, "constructor", ValueError, "needs UnetRes(num_unet=2)"
    if obj in ("pred_res", "pred_noise"):
        return RAISES, "_plan", ValueError, f"objective {obj!r} with num_unet=2"
    if obj == "pred_x0_noise":
        if tst == "res_noise":
            return (3, True, True, 0), False, 16
        return RAISES, "_plan", ValueError, "must be 'res_noise'"
    return {"res": ((0, True, False, 0), True, 32), "noise": ((1, False, True, 0), False, 32),
            "res_noise": ((2, True, True, 0), False, 16),
            # a known wart, pinned and left alone: every neighbouring case raises a ValueError that names the problem, the sampler's
            # default test_res_or_noise="None" on a two-U-Net 'pred_res_noise' model a bare KeyError
            "None": (RAISES, "_plan", KeyError, "'None'")}[tst]


NETS = {}


def _net(nu):
    if nu not in NETS:
        NETS[nu] = UnetRes(dim=32, dim_mults=(1, 2), clip_cfg=TINY_CLIP, num_unet=nu, condition=True)
    return NETS[nu]


def _dif(nu, obj, tst):
    dif = ResidualDiffusion(_net(nu), image_size=8, sampling_timesteps=3, objective=obj, condition=True, test_res_or_noise=tst)
    dif.streams, dif.max_sub_batch = 2, 16                     # the defaults, whatever the environment says
    return dif


@pytest.mark.parametrize("nu,obj,tst", list(itertools.product((1, 2), OBJECTIVES, TESTS)))
def test_a1_sampling_plan_of_every_combination(nu, obj, tst):
    want = _expected_plan(nu, obj, tst)
    if want[0] == RAISES and want[1] == "constructor":
        with pytest.raises(want[2]) as e:
            _dif(nu, obj, tst)
        assert want[3] in str(e.value)
        return
    dif = _dif(nu, obj, tst)
    if want[0] == RAISES:
        for call in (dif._plan, dif._is_shipped, dif._group_rows):
            with pytest.raises(want[2]) as e:
                call()
            assert type(e.value) is want[2] and want[3] in str(e.value)
        return
    plan, shipped, group = want
    assert dif._plan() == plan and tuple(dif._plan()) == plan
    assert dif._is_shipped() is shipped
    assert dif._group_rows() == group
    assert [u is dif.model.unet0 for u in dif._plan_unets()] == [True] * plan[1] + [False] * plan[2]


def test_a1_unknown_objective_and_the_third_plane():
    with pytest.raises(ValueError, match="unknown objective 'pred_x0'"):
        ResidualDiffusion(_net(1), image_size=8, objective="pred_x0", condition=True)
    dif = _dif(1, "pred_res", "res")
    dif.input_condition = True                                 # the shipped plan on a 3-plane model is not the shipped path
    assert dif._plan() == (0, True, False, 0) and not dif._is_shipped() and not dif._captured_plan()


# ---- A2: UnetRes.forward.  The U-Nets' forwards are recorders; time = [a, b]
A, B_ = torch.tensor([1.0]), torch.tensor([2.0])


def _recording_net(nu, obj, tst):
    net = UnetRes(dim=32, dim_mults=(1, 2), clip_cfg=TINY_CLIP, num_unet=nu, condition=True, objective=obj, test_res_or_noise=tst)
    calls = []

    def recorder(name, kind):
        def run(x, time, **kw):
            which = "a" if time is A else "b" if time is B_ else "?"
            calls.append((name, kind, which, tuple(sorted(kw))))
            return (name, kind)
        return run
    for name, u in zip(("unet0", "unet1"), net._unets()):
        u.forward, u.train_forward = recorder(name, "engine"), recorder(name, "train")
    return net, calls


KW = ("reuse_condition", "x_self_cond")
# (num_unet, objective, test_res_or_noise) -> (what comes back, the calls) under no_grad
INFER = {
    (2, "res_noise"): ((("unet0", "engine"), ("unet1", "engine")), [("unet0", "engine", "a", KW), ("unet1", "engine", "b", KW)]),
    (2, "res"): ((("unet0", "engine"), 0), [("unet0", "engine", "a", KW)]),
    (2, "noise"): ((0, ("unet1", "engine")), [("unet1", "engine", "b", KW)]),
    (1, "pred_res"): ([("unet0", "engine")], [("unet0", "engine", "a", KW)]),
    (1, "pred_noise"): ([("unet0", "engine")], [("unet0", "engine", "b", KW)]),
}


# every objective on two U-Nets, those of one U-Net included: under no_grad the two-U-Net branch never looks at the objective
@pytest.mark.parametrize("nu,obj,tst", [c for c in itertools.product((1, 2), OBJECTIVES, TESTS)
                                        if c[0] == 2 or c[1] in ("pred_res", "pred_noise")])
def test_a2_unetres_forward_under_no_grad(nu, obj, tst):
    net, calls = _recording_net(nu, obj, tst)
    with torch.no_grad():
        if nu == 2 and tst == "None":
            with pytest.raises(ValueError, match="test_res_or_noise='None'"):
                net(None, [A, B_])
            assert calls == []
            return
        out = net(None, [A, B_])
    want, want_calls = INFER[(2, tst) if nu == 2 else (1, obj)]
    assert type(out) is type(want) and len(out) == len(want) and out == want
    assert calls == want_calls


# objective -> the training forwards, in the order of the list that comes back
TRAIN = {"pred_res": [("unet0", "train", "a", ())], "pred_noise": [("unet0", "train", "b", ())],
         "pred_res_noise": [("unet0", "train", "a", ()), ("unet1", "train", "b", ())],
         "pred_x0_noise": [("unet0", "train", "a", ()), ("unet1", "train", "b", ())]}


@pytest.mark.parametrize("obj", OBJECTIVES)
def test_a2_unetres_forward_under_gradients(obj):
    nu = len(TRAIN[obj])
    net, calls = _recording_net(nu, obj, "res_noise")
    with torch.enable_grad():
        assert net(None, [A, B_]) == ([("unet0", "engine")] if nu == 1 else (("unet0", "engine"), ("unet1", "engine")))
        calls.clear()                                          # (no trainable view: the engine, even under gradients)
        for u in net._unets():
            u._trainable = object()
        out = net(None, [A, B_])
    assert type(out) is list and out == [c[:2] for c in TRAIN[obj]] and calls == TRAIN[obj]
    with torch.no_grad():                                      # a model that trains still samples under no_grad
        calls.clear()
        net(None, [A, B_])
        assert [c[1] for c in calls] == ["engine"] * nu


def test_a2_unetres_forward_refusals():
    for missing in (0, 1):                                     # one of two views missing
        net, calls = _recording_net(2, "pred_res_noise", "res_noise")
        net._unets()[1 - missing]._trainable = object()
        with torch.enable_grad(), pytest.raises(NotImplementedError, match="one of the two has no trainable view"):
            net(None, [A, B_])
        assert calls == []
    for nu, obj, text in ((2, "pred_res", "needs num_unet=1"), (2, "pred_noise", "needs num_unet=1"),
                          (1, "pred_res_noise", "needs num_unet=2"), (1, "pred_x0_noise", "needs num_unet=2")):
        net, calls = _recording_net(nu, obj, "res_noise")
        for u in net._unets():
            u._trainable = object()
        with torch.enable_grad(), pytest.raises(ValueError) as e:
            net(None, [A, B_])
        assert f"objective {obj!r} {text} (src/DADiff.py:826-831)" == str(e.value) and calls == []
    net, calls = _recording_net(1, "pred_res_noise", "res_noise")
    with torch.no_grad(), pytest.raises(ValueError, match="needs num_unet=2"):
        net(None, [A, B_])
    assert calls == []


# ---- A3: diffusion_train.p_losses_fn.  q_sample, its argument checks and residual_loss are stubs
# objective -> (x0_out asked of q_sample, the target of each model output)
LOSSES = {"pred_res": (False, ["x_res"]), "pred_noise": (False, ["noise"]), "pred_res_noise": (False, ["x_res", "noise"]),
          "pred_x0_noise": (True, ["x0", "noise"])}


@pytest.fixture
def qsample_stubs(monkeypatch):
    log = {"q_sample": [], "checks": []}

    def q_sample(x_start, x_input, t, schedule, noise=None, slice_seeds=None, step=0, normalize=True, x0_out=False):
        log["q_sample"].append(dict(x_start=x_start, x_input=x_input, normalize=normalize, x0_out=x0_out))
        x_in = torch.zeros(2, 2, 4, 4)
        return (x_in, "x_res", "noise", ("time0", "time1")) + (("x0",) if x0_out else ())
    monkeypatch.setattr(dt, "q_sample", q_sample)
    monkeypatch.setattr(dt, "_check_qsample", lambda fn, *a, **k: log["checks"].append((fn, "tensors", k.get("dims"))))
    monkeypatch.setattr(dt, "_check_qsample_store", lambda fn, *a, **k: log["checks"].append((fn, "store")))
    monkeypatch.setattr(dt, "residual_loss", lambda pred, target, loss_type, scale=1.0: (pred, target, loss_type, scale))
    monkeypatch.setattr(dt, "val_items", lambda pred, target, loss_type, *res: (pred, target, loss_type, res))
    return log


@pytest.mark.parametrize("obj", OBJECTIVES)
@pytest.mark.parametrize("store", (False, True))
def test_a3_p_losses_targets(qsample_stubs, obj, store):
    want_x0, targets = LOSSES[obj]
    seen = []

    def model_fn(x_in, times):
        seen.append(times)
        return [f"out{i}" for i in range(len(targets))]
    imgs = object.__new__(dt.StoreBatch) if store else ["x_start", "x_input"]
    out = dt.p_losses_fn(model_fn, imgs, "t", {}, obj, "l2", scale=0.5, normalize=True)
    assert out == [(f"out{i}", tg, "l2", 0.5) for i, tg in enumerate(targets)]
    assert seen == [["time0", "time1"]]
    (q,) = qsample_stubs["q_sample"]
    assert q["x0_out"] is want_x0 and q["normalize"] is True
    assert (q["x_start"], q["x_input"]) == ((imgs, None) if store else ("x_start", "x_input"))
    assert qsample_stubs["checks"] == ([("p_losses", "store")] if store else [("p_losses", "tensors", (4,))])


def test_a3_p_losses_refusals(qsample_stubs):
    two = lambda x_in, times: ["out0"]
    with pytest.raises(RuntimeError) as e:
        dt.p_losses_fn(two, ["x_start", "x_input"], "t", {}, "pred_res_noise")
    assert str(e.value) == "p_losses: objective 'pred_res_noise' needs 2 model output(s) (got 1)"
    with pytest.raises(RuntimeError) as e:
        dt.p_losses_fn(lambda x_in, times: "out", ["x_start", "x_input"], "t", {}, "pred_noise")
    assert str(e.value) == "p_losses: objective 'pred_noise' needs 1 model output(s) (got str)"
    diffused = len(qsample_stubs["q_sample"])                  # the two below are refused before anything is diffused
    with pytest.raises(RuntimeError) as e:
        dt.p_losses_fn(two, ["x_start", "x_input"], "t", {}, "pred_x0")
    assert str(e.value) == "p_losses: unknown objective 'pred_x0'"
    with pytest.raises(RuntimeError, match="p_losses: imgs must be \\[x_start, x_input\\]"):
        dt.p_losses_fn(two, "x_start", "t", {}, "pred_res")
    assert len(qsample_stubs["q_sample"]) == diffused == 2


# ---- A4: ResidualDiffusion.eval_items.  The engines are stubs; q_sample and val_items those of A3
# objective -> per U-Net (its name, its time input, its target, whether (x_input, x0) go to val_items as the residual's arguments)
EVAL = {"pred_res": [("unet0", "time0", "x_res", True)], "pred_noise": [("unet0", "time1", "noise", False)],
        "pred_res_noise": [("unet0", "time0", "x_res", True), ("unet1", "time1", "noise", False)],
        "pred_x0_noise": [("unet0", "time0", "x0", False), ("unet1", "time1", "noise", False)]}


class _NoDevice:
    def __init__(self, device):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


@pytest.mark.parametrize("obj", OBJECTIVES)
@pytest.mark.parametrize("store", (False, True))
def test_a4_eval_items_routing(qsample_stubs, monkeypatch, obj, store):
    monkeypatch.setattr(torch.cuda, "device", _NoDevice)
    nu = len(EVAL[obj])
    dif = _dif(nu, obj, "res_noise")
    rows = []

    class Engine:
        def __init__(self, name, precision):
            self.name, self.precision = name, precision

        def encode_condition(self, x_input):
            rows.append(("encode_condition", self.name, tuple(x_input.shape)))

        def forward(self, x_t, x_input, time):
            rows.append(("forward", self.name, self.precision, time))
            return "pred:" + self.name
    for name, u in zip(("unet0", "unet1"), dif.model._unets()):       # (the nets are shared: monkeypatch puts the method back)
        monkeypatch.setattr(u, "engine", (lambda n: lambda precision=None, slot=0: Engine(n, precision))(name), raising=False)
    imgs = object.__new__(dt.StoreBatch) if store else ["x_start", "x_input"]
    out = dif.eval_items(imgs, "t", precision="fp32s")
    (q,) = qsample_stubs["q_sample"]
    assert q["x0_out"] is True and q["normalize"] is True
    fn = "ResidualDiffusion.eval_items"
    assert qsample_stubs["checks"] == ([(fn, "store")] if store else [(fn, "tensors", (4,))])
    assert [r[1:] for r in rows if r[0] == "forward"] == [(name, "fp32s", time) for name, time, _, _ in EVAL[obj]]
    assert [r[1] for r in rows if r[0] == "encode_condition"] == [name for name, _, _, _ in EVAL[obj]]
    assert len(out) == nu
    for (pred, target, loss_type, res), (name, _, want, residual) in zip(out, EVAL[obj]):
        assert pred == "pred:" + name and target == want and loss_type == "l1"
        assert len(res) == (2 if residual else 0)
        if residual:
            assert tuple(res[0].shape) == (2, 1, 4, 4) and res[1] == "x0"           # (x_input, x0)
    with pytest.raises(RuntimeError, match="ResidualDiffusion.eval_items: imgs must be \\[x_start, x_input\\]"):
        dif.eval_items("x_start", "t")


# ---- Part B: founddiff_amd/objectives.py itself
TARGET_NAMES = {"x_res": "res", "noise": "noise", "x0": "x0"}     # Part A's stubs name q_sample's results; the table names targets


def test_b_training_table_is_what_part_a_records():
    from founddiff_amd import objectives as O
    assert tuple(O.TRAINING) == OBJECTIVES
    assert [len(O.TRAINING[o]) for o in OBJECTIVES] == [1, 1, 2, 2]
    for obj in OBJECTIVES:
        rows = [tuple(r) for r in O.TRAINING[obj]]
        assert rows == [(int(name[-1]), int(time[-1]), TARGET_NAMES[tg], residual) for name, time, tg, residual in EVAL[obj]]
        assert [r[2] for r in rows] == [TARGET_NAMES[tg] for tg in LOSSES[obj][1]]
        assert [(f"unet{r[0]}", "train", "ab"[r[1]], ()) for r in rows] == TRAIN[obj]
        assert all(r.target in ("res", "noise", "x0") and isinstance(r.residual, bool) for r in O.TRAINING[obj])


@pytest.mark.parametrize("nu,obj,tst", list(itertools.product((1, 2), OBJECTIVES, TESTS)))
def test_b_sample_plan_agrees_with_part_a_and_the_training_table(nu, obj, tst):
    from founddiff_amd import objectives as O
    want = _expected_plan(nu, obj, tst)
    if want[0] == RAISES and want[1] == "constructor":
        with pytest.raises(want[2]) as e:
            O.check_model(obj, nu)
        assert want[3] in str(e.value)
        return
    O.check_model(obj, nu)
    if want[0] == RAISES:
        with pytest.raises(want[2]) as e:
            O.sample_plan(obj, nu, tst)
        assert type(e.value) is want[2] and want[3] in str(e.value)
        return
    plan = O.sample_plan(obj, nu, tst)
    assert plan == want[0] and hash(plan) == hash(want[0]) and {plan: 1}[want[0]] == 1
    assert isinstance(plan, tuple) and (plan.mode, plan.run0, plan.run1, plan.time0) == want[0]
    assert list(plan) == list(want[0]) and plan + (3,) == want[0] + (3,)            # (_obj_key extends it, JSON lists it)
    assert plan.two_engines is (want[2] == 16)
    # the U-Nets the plan runs are among those the objective trains, at the same time input
    trained = {r.unet: r.time for r in O.TRAINING[obj]}
    assert set(plan.unets) <= set(trained) and plan.unets == tuple(i for i, r in enumerate((plan.run0, plan.run1)) if r)
    for i in plan.unets:
        assert plan.times[i] == trained[i] == (plan.time0 if i == 0 else 1)
    assert [plan.times[i] for i in (0, 1) if i not in plan.unets] == [None] * (2 - len(plan.unets))
    # (o0, o1) from the raw outputs, in the order of plan.unets
    outs = [f"out{i}" for i in plan.unets]
    o0, o1 = plan.o01(outs)
    if plan.mode == 1:
        assert (o0, o1) == (None, outs[0])                     # the noise is the step kernels' o1, whichever U-Net predicts it
    else:
        assert (o0, o1) == ("out0" if plan.run0 else None, "out1" if plan.run1 else None)


def test_b_checks_keep_their_texts():
    from founddiff_amd import objectives as O
    with pytest.raises(ValueError) as e:
        O.check_objective("pred_x0")
    assert str(e.value) == "unknown objective 'pred_x0'"
    with pytest.raises(RuntimeError) as e:
        O.check_objective("pred_x0", RuntimeError, "p_losses: ")
    assert str(e.value) == "p_losses: unknown objective 'pred_x0'"
    with pytest.raises(ValueError) as e:
        O.check_model("pred_x0_noise", 1)
    assert str(e.value) == "objective 'pred_x0_noise' needs UnetRes(num_unet=2) (src/DADiff.py:826-831)"
    with pytest.raises(ValueError) as e:
        O.routed("pred_res", 2)
    assert str(e.value) == "objective 'pred_res' needs num_unet=1 (src/DADiff.py:826-831)"
    assert O.routed("pred_noise", 1) is O.TRAINING["pred_noise"]

    class Stub:                                                # a model that is no UnetRes: one U-Net, no num_unet
        unet0 = "u0"
    assert O.unets_of(Stub()) == ["u0"] and O.num_unet(Stub()) == 1 and O.unets_of(None) == []
    assert O.unets_of(_net(2)) == _net(2)._unets() and O.num_unet(_net(2)) == 2


def _child(code):
    return subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)


def test_b_objectives_is_pure_host_code():
    r = _child("import sys, founddiff_amd.objectives; "
               "print(sorted(m for m in ('torch', 'numpy', 'founddiff_amd._lib', 'founddiff_amd.DADiff') if m in sys.modules))")
    assert r.returncode == 0 and r.stdout.strip() == "[]", r.stdout + r.stderr


def test_b_trainer_is_a_module_of_its_own():
    r = _child("import sys, founddiff_amd.trainer as T; assert 'founddiff_amd.DADiff' not in sys.modules; "
               "import founddiff_amd.DADiff as D; assert D.Trainer is T.Trainer and D.load_weights is T.load_weights; print('ok')")
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
    import founddiff_amd.DADiff as D
    import founddiff_amd.trainer as T
    assert D.Trainer is T.Trainer and D._EMAView is T._EMAView and D._Accel is T._Accel and D._QuantilePlan is T._QuantilePlan
