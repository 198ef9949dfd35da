"""The objective routing rule, stated once: given `objective`, `num_unet` and `test_res_or_noise`, which U-Net runs, at which of the
two time inputs, predicting what (reference src/DADiff.py:817-836 UnetRes.forward, 1168-1207 model_predictions, 1399-1482 p_losses).

    TRAINING       objective -> one Row per U-Net it trains.  UnetRes.forward, diffusion_train.p_losses_fn and
                   ResidualDiffusion.eval_items route, and pick their targets, from these rows
    sample_plan    (objective, num_unet, test_res_or_noise) -> SamplePlan: the rows that run when sampling and the mode of the step
                   kernels for them.  ResidualDiffusion._plan() returns it; the samplers read its members
    the checks     check_objective, check_model, routed: the refusals of an objective, and of an objective on a model
    the model      UNET_NAMES, unets_of, num_unet: "the U-Nets of this model" for anything shaped like a UnetRes

Pure host code: it imports neither torch nor the library, and is the same on a machine without a GPU.
"""
from typing import NamedTuple

UNET_NAMES = ("unet0", "unet1")


class Row(NamedTuple):
    """One U-Net of an objective: its index, which of the two time inputs it reads (0: alphas_cumsum[t] T, 1: betas_cumsum[t] T),
    what it predicts ("res", "noise" or "x0") and whether that output is a residual, i.e. clamp(x_input - clamp(output)) is a
    one-step estimate of x_start."""
    unet: int
    time: int
    target: str
    residual: bool


TRAINING = {
    "pred_res": (Row(0, 0, "res", True),),
    "pred_noise": (Row(0, 1, "noise", False),),
    "pred_res_noise": (Row(0, 0, "res", True), Row(1, 1, "noise", False)),
    "pred_x0_noise": (Row(0, 0, "x0", False), Row(1, 1, "noise", False)),
}
TWO_UNETS = tuple(o for o, rows in TRAINING.items() if len(rows) == 2)
ONE_UNET_TEXT = "'pred_res' and 'pred_noise'"      # the objectives of one U-Net, as the refusal to train two untrained ones names them
SHIPPED = "pred_res"             # the objective of the shipped checkpoints: its plan has loops and kernels of its own
# test_res_or_noise -> the U-Nets of a two-U-Net model that run under no_grad.  There U-Net i reads time input i whatever the
# objective (src/DADiff.py:817-823), which is what the rows of the two-U-Net objectives say too
TEST_UNETS = {"res_noise": (0, 1), "res": (0,), "noise": (1,)}
# what the U-Nets that run predict -> the mode of fd_res_step_obj and its kin
_MODES = {("res",): 0, ("noise",): 1, ("res", "noise"): 2, ("x0", "noise"): 3}
_REF = "(src/DADiff.py:826-831)"


# ---- the model
def unets_of(model):
    """Every U-Net `model` has, unet0 first.  Duck-typed: a UnetRes, or anything with a `unet0` (and maybe a `unet1`)."""
    return [u for u in (getattr(model, n, None) for n in UNET_NAMES) if u is not None]


def num_unet(model):
    return getattr(model, "num_unet", 1)


# ---- the checks
def check_objective(objective, error=ValueError, prefix=""):
    if objective not in TRAINING:
        raise error(f"{prefix}unknown objective {objective!r}")


def check_model(objective, n):
    """the sampler's constructor: an objective of two U-Nets on a model that does not have two"""
    if objective in TWO_UNETS and n != 2:
        raise ValueError(f"objective {objective!r} needs UnetRes(num_unet=2) {_REF}")


def routed(objective, n):
    """The rows of `objective` on a model of `n` U-Nets; ValueError where the two do not pair."""
    rows = TRAINING.get(objective, ())
    if len(rows) != n:
        raise ValueError(f"objective {objective!r} needs num_unet={1 if n == 2 else 2} {_REF}")
    return rows


# ---- sampling
class SamplePlan(NamedTuple):
    """(mode of fd_res_step_obj, run unet0?, run unet1?, unet0's time entry): a plain tuple to whatever compares, hashes or lists
    it (the graph keys do), with the readings of it that the samplers need."""
    mode: int
    run0: bool
    run1: bool
    time0: int

    @property
    def unets(self):
        """the indices of the U-Nets this plan evaluates, unet0 first"""
        return tuple(i for i, run in enumerate((self.run0, self.run1)) if run)

    @property
    def two_engines(self):
        """two engines per stream: each then holds half the slices one would"""
        return self.run0 and self.run1

    @property
    def times(self):
        """per U-Net the time input it is fed (0: alphas_cumsum, 1: betas_cumsum), None where the plan does not run it"""
        return (self.time0 if self.run0 else None, 1 if self.run1 else None)

    def o01(self, outs):
        """(o0, o1) as the step kernels take them, from the raw outputs of the plan's U-Nets in the order of `unets`.  o1 is the
        predicted noise, whichever U-Net predicts it: a single U-Net in mode 1 fills o1."""
        if self.mode == 1 and self.run0:
            return None, outs[0]
        return outs[0] if self.run0 else None, outs[-1] if self.run1 else None


def sample_plan(objective, n, test_res_or_noise):
    """The SamplePlan of a model of `n` U-Nets.  Two U-Nets: the rows test_res_or_noise selects; 'x0' cannot be sampled alone.
    One U-Net: its objective's only row (the constructor has refused the objectives of two, which would sample as the shipped
    one)."""
    if n == 2:
        rows = TRAINING.get(objective, ())
        if len(rows) != 2:
            raise ValueError(f"objective {objective!r} with num_unet=2")
        if any(r.target == "x0" for r in rows) and test_res_or_noise != "res_noise":
            raise ValueError(f"{objective} reads both model outputs: test_res_or_noise must be 'res_noise'")
        # known wart, pinned by tests/test_objectives_cpu.py: the sampler's default "None" ends here in a bare KeyError
        run = [rows[i] for i in TEST_UNETS[test_res_or_noise]]
    else:
        rows = TRAINING.get(objective, ())
        run = list(rows if len(rows) == 1 else TRAINING[SHIPPED])
    ran = {r.unet: r.time for r in run}
    return SamplePlan(_MODES[tuple(r.target for r in run)], 0 in ran, 1 in ran, ran.get(0, 0))


SHIPPED_PLAN = sample_plan(SHIPPED, 1, None)
