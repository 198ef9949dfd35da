"""Drop-in mirror of the reference's `src/DADiff.py` sampling API, executed on MI355X HIP kernels.

    from founddiff_amd.DADiff import ResidualDiffusion, Trainer, Unet, UnetRes, set_seed

Same class names, constructor kwargs, method names/signatures and state_dict key layout as the
reference (`/root/reference/src/DADiff.py`; contract in SURVEY.md section 8b), so
`checkpoints/<name>/sample/model-N.pt` loads unchanged.  The modules below hold parameters only:
`forward` never runs a torch op on activations -- it hands device pointers to libfounddiff_hip.so
through `founddiff_amd.engine.DAEngine`.  What the reference does not have -- `sample_ensemble`, `sample_tiled`, their results
`EnsembleResult` / `EnsembleQuantiles` -- is `founddiff_amd/tiled_sampling.py`, a mixin of `ResidualDiffusion`.

This file holds the parameter-only `Unet` / `UnetRes`, the `ResidualDiffusion` sampler and its training entry points (`forward`,
`p_losses`, `eval_items`).  Three things it used to hold live beside it and are imported from here as before:
`founddiff_amd/objectives.py` states the routing rule once -- which U-Net runs, at which time input, predicting what, per objective,
`num_unet` and `test_res_or_noise` -- and `UnetRes.forward`, `ResidualDiffusion._plan` and `eval_items` read it;
`founddiff_amd/trainer.py` is the `Trainer` with `_Accel` and `_EMAView`; `founddiff_amd/schedule.py` is `residual_schedule` and
`load_weights`, which the sampler and the Trainer share.

Training runs on the same classes: `Unet.trainable()` is a `unet_train.UnetTrunk` over the very
parameters of the tree, `Unet.train_forward` runs the frozen DA-CLIP tower on the fp32 engine and the trunk under autograd on the HIP
training kernels, `ResidualDiffusion.forward` / `p_losses` are the reference's (diffusion_train), and `Trainer.train / save / load`
(trainer.py) are its loop and checkpoint around `diffusion_train.ClipAdamEMA`.  Two U-Nets, which the reference optimises with RAdam, train
around `diffusion_train.ClipRAdamEMA` on request: `UnetRes.trainable()` and `Trainer(optimizer="radam")`; the defaults raise.
"""
import copy
import math
import os
import random
from collections import namedtuple

import numpy as np
import torch
from torch import nn

from . import _lib as L
from . import arch
from . import diffusion_train as dt
from . import objectives
from .engine import DAEngine, _p
from .schedule import load_weights, residual_schedule  # noqa: F401 (load_weights is imported from here)
from .tiled_sampling import EnsembleQuantiles, EnsembleResult, TiledSampling  # noqa: F401 (the results are imported from here)
from .trainer import Trainer, _Accel, _EMAView, _QuantilePlan  # noqa: F401 (the reference's names: they are imported from here)

ModelResPrediction = namedtuple("ModelResPrediction", ["pred_res", "pred_noise", "pred_x_start"])


def set_seed(SEED):
    """src/DADiff.py:65-70"""
    torch.manual_seed(SEED)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(SEED)
    np.random.seed(SEED)
    random.seed(SEED)


def exists(x):
    return x is not None


def default(val, d):
    if exists(val):
        return val
    return d() if callable(d) else d


def normalize_to_neg_one_to_one(img):
    if isinstance(img, list):
        return [_affine(t, 2.0, -1.0) for t in img]
    return _affine(img, 2.0, -1.0)


def unnormalize_to_zero_to_one(img):
    if isinstance(img, list):
        return [_affine(t, 0.5, 0.5) for t in img]
    return _affine(img, 0.5, 0.5)


def _stream(t):
    import ctypes as C
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _affine(x, a, b):
    x = x.contiguous().float()
    out = torch.empty_like(x)
    L.call("fd_affine_f32", _p(x), a, b, _p(out), x.numel(), _stream(x))
    return out


class _ParamTree(nn.Module):
    """Parameter container reproducing a flat {dotted.key: shape} layout as nested modules."""

    def _attach(self, key, shape, dtype=torch.float32, buffer=False):
        parts = key.split(".")
        mod = self
        for p in parts[:-1]:
            if not hasattr(mod, p):
                mod.add_module(p, _ParamTree())
            mod = getattr(mod, p)
        if buffer or dtype != torch.float32:
            mod.register_buffer(parts[-1], torch.zeros(shape, dtype=dtype))
        else:
            mod.register_parameter(parts[-1], nn.Parameter(torch.zeros(shape), requires_grad=False))


def _build_tree(root, spec):
    for k, s in spec.items():
        if isinstance(s, tuple) and len(s) == 2 and isinstance(s[1], str):
            root._attach(k, s[0], getattr(torch, s[1]), buffer=True)
        else:
            leaf = k.rsplit(".", 1)[-1]
            root._attach(k, s, buffer=leaf in ("running_mean", "running_var"))


class Unet(_ParamTree):
    """DA-CLIP conditioned U-Net (reference src/DADiff.py:530-740).  `condition` is forced on
    as in the reference (line 586).  Extra kwargs: `precision` selects the kernel mode -- 'bf16' (default) | 'fp16' (the same kernels
    on the library's IEEE-binary16 build: 8 x smaller drift at 0.96 of the speed, binary16's range) | 'auto' ('fp16' until a sample()
    leaves that range, 'bf16' from then on) | 'fp32s' | 'fp32' | 'fp8' (bf16
    kernels with e4m3 weights on the fp8 MFMA for the 3x3 convolutions, BASELINE configs[4]); `clip_cfg` overrides the RN50 DA-CLIP geometry (tests use a shrunken one)."""

    def __init__(self, dim, init_dim=None, out_dim=None, dim_mults=(1, 2, 4, 8), channels=1,
                 self_condition=False, resnet_block_groups=8, learned_variance=False,
                 learned_sinusoidal_cond=False, random_fourier_features=False, learned_sinusoidal_dim=16,
                 condition=False, input_condition=False, precision=None, clip_cfg=None):
        super().__init__()
        if self_condition or learned_variance or learned_sinusoidal_cond or \
                random_fourier_features or resnet_block_groups != 8 or (init_dim not in (None, dim)) or channels != 1:
            raise NotImplementedError("Unet is built for channels=1, condition=True, no self-conditioning / learned "
                                      "variance / learned sinusoidal embedding (SURVEY 8f-4)")
        self.input_condition = input_condition
        self.channels = channels
        self.self_condition = self_condition
        self.dim, self.dim_mults = dim, tuple(dim_mults)
        self.out_dim = default(out_dim, channels)
        self.random_or_learned_sinusoidal_cond = False
        self.precision = precision or os.environ.get("FOUNDDIFF_PRECISION", "bf16")
        self._auto_bf16 = False          # precision='auto': set once a sample() left binary16's range (ResidualDiffusion.sample)
        # kernel set for one slice at a time (DAEngine low_latency); Trainer.test(batch_size=1) turns it on
        self.low_latency = bool(int(os.environ.get("FOUNDDIFF_LOW_LATENCY", "0")))
        self.clip_cfg = clip_cfg or arch.RN50
        _build_tree(self, arch.da_unet_spec(dim, self.dim_mults, channels, "", self.clip_cfg, input_condition))
        self._engine = None

    _trainable = None        # trainable()'s UnetTrunk; kept out of _modules, so state_dict() and .to() meet every parameter once
    _train_engine = None     # the 'fp32' engine of train_forward: the frozen DA-CLIP tower alone (DAEngine(tower_only=True))

    def _drop_engines(self):
        """every packed copy of the weights, the frozen tower's included: the parameters were replaced or moved"""
        self._engine = None
        self._train_engine = None

    # --- checkpoint handling: accept-and-ignore the dead weight a real checkpoint carries
    def load_state_dict(self, state_dict, strict=True, assign=False):
        live = {k: v for k, v in state_dict.items() if not arch.is_dead_key("unet0." + k, "unet0.")}
        self._drop_engines()
        if assign:                       # new Parameter objects: the view would keep the old ones
            self.__dict__.pop("_trainable", None)
        return super().load_state_dict(live, strict=strict, assign=assign)

    def _load_from_state_dict(self, *a, **k):
        self._drop_engines()
        return super()._load_from_state_dict(*a, **k)

    def _apply(self, fn, *a, **k):
        # .to(device) / .cuda() / dtype casts move the parameters: the packed weights of the engine are stale
        self._drop_engines()
        return super()._apply(fn, *a, **k)

    # --- training
    def weights_changed(self):
        """Tell the model that its trunk parameters were written in place behind its back (ClipAdamEMA writes through raw pointers):
        the packed engines and the graphs they captured are dropped, the next sampling call packs again.  The engine of
        train_forward stays: it holds the frozen tower only."""
        self._engine = None

    def trainable(self):
        """The trunk of this model as a unet_train.UnetTrunk, built once: its parameters ARE the nn.Parameter objects of this tree's
        trunk entries (re-registered, not copied), so state_dict(), .to(), load_state_dict() and the engines' packing see the same
        storage.  Trunk parameters get requires_grad=True; everything under dose_encoder. stays frozen.  From the first call on
        UnetRes.forward routes to train_forward whenever gradients are enabled."""
        if self._trainable is None:
            if self.input_condition or self.self_condition:
                raise RuntimeError("Unet.trainable: input_condition and self_condition are not supported in training")
            from .unet_train import UnetTrunk
            with torch.random.fork_rng(devices=[]):           # the view's own initialisation is thrown away: leave the generator alone
                trunk = UnetTrunk(self.dim, self.dim_mults, channels=self.channels, input_channels=2 * self.channels)
            mine = {k: p for k, p in self.named_parameters() if not k.startswith("dose_encoder.")}
            theirs = [k for k, _ in trunk.named_parameters()]
            if set(theirs) != set(mine) or any(trunk.get_parameter(k).shape != mine[k].shape for k in theirs):
                odd = sorted(set(theirs) ^ set(mine)) or [k for k in theirs if trunk.get_parameter(k).shape != mine[k].shape]
                raise RuntimeError(f"Unet.trainable: the trunk's layout differs from UnetTrunk's (e.g. {odd[:3]})")
            for k in theirs:
                parent, _, leaf = k.rpartition(".")
                trunk.get_submodule(parent)._parameters[leaf] = mine[k].requires_grad_(True)
            self.__dict__["_trainable"] = trunk
        return self._trainable

    def train_forward(self, x, time):
        """x (B, 2, H, W) = cat(x_t, x_input), time (B,) -> (B, 1, H, W), differentiable in the trunk's parameters.  The frozen DA-CLIP
        tower runs on this model's 'fp32' engine whatever its sampling precision (the reference trains in fp32); the trunk, the two
        outer convolutions included, on the HIP training kernels (unet_train.unet_trunk_forward)."""
        from .outer_conv_train import final_conv_fn, init_conv_fn
        from .unet_train import unet_trunk_forward
        fn = "Unet.train_forward"
        trunk = self.trainable()
        for name, v in (("x", x), ("time", time)):
            if not isinstance(v, torch.Tensor):
                raise RuntimeError(f"{fn}: {name} must be a tensor (got {type(v).__name__})")
        if x.dim() != 4 or x.shape[1] != 2 * self.channels or time.dim() != 1 or time.shape[0] != x.shape[0]:
            raise RuntimeError(f"{fn}: inconsistent shapes x{tuple(x.shape)} time{tuple(time.shape)} (expected (B, 2, H, W) and (B,))")
        if not x.is_cuda or not time.is_cuda or next(self.parameters()).device != x.device:
            raise RuntimeError(f"{fn}: x, time and the model must live on one GPU (there is no CPU path)")
        x = x.detach().float().contiguous()
        if self._train_engine is None:
            tower = {k: v for k, v in self.state_dict().items() if k.startswith("dose_encoder.")}
            self._train_engine = DAEngine(tower, "", x.device, "fp32", tower_only=True)      # no copy of the trunk: it would go stale
        with torch.no_grad(), torch.cuda.device(x.device):
            dose, ctx = self._train_engine.encode_dose(x[:, 1:2].contiguous())
            dose, ctx = dose.clone(), ctx.clone()             # the engine's buffers belong to its next call
        return unet_trunk_forward(trunk, x, time.float(), dose, ctx.unsqueeze(1), init_fn=init_conv_fn, final_fn=final_conv_fn)

    def load_dose_clip(self, path_or_state="Dose-CLIP.pth"):
        """The reference builds its dose encoder from a separate file at construction time:
        `clipiqa.load_state_dict(torch.load('Dose-CLIP.pth'), strict=True)` (src/DADiff.py:595-596).  A
        `model-N.pt` checkpoint carries the same tensors under `dose_encoder.*`, so this is only needed for a
        model that is not loaded from a checkpoint.  Strict on every key that is live on the sampling path (the
        RN50 visual tower + head1 / head2); the text tower and prompt learner of the file are dead weight."""
        sd = path_or_state
        if not isinstance(sd, dict):
            sd = torch.load(str(sd), map_location="cpu", weights_only=False)
        mine = {k for k in self.state_dict() if k.startswith("dose_encoder.")}
        live = {"dose_encoder." + k: v for k, v in sd.items() if "dose_encoder." + k in mine}
        missing = sorted(mine - set(live))
        if missing:
            raise RuntimeError(f"Dose-CLIP state_dict lacks {len(missing)} live keys, e.g. {[m[len('dose_encoder.'):] for m in missing[:3]]}")
        res = super().load_state_dict(live, strict=False)
        assert not res.unexpected_keys
        self._drop_engines()
        return res

    @property
    def kernel_precision(self):
        """the kernel mode `precision` stands for: 'auto' = 'fp16' (the 16-bit kernels on the binary16 build: 8 x smaller drift than
        'bf16' at 0.96 of its speed) until a sample() of this model has produced a non-finite image -- an activation beyond binary16's
        65504 -- and 'bf16' from then on"""
        if self.precision == "auto":
            return "bf16" if self._auto_bf16 else "fp16"
        return self.precision

    def engine(self, precision=None, slot=0):
        """The packed-weight HIP engine of this UNet for `precision` (default: self.precision); one per
        precision is kept (the samplers run their last step(s) on the fp32 engine, see ResidualDiffusion).
        `slot`: engines with their own workspaces for concurrent half-batches (ResidualDiffusion.sample)."""
        prec = precision or self.kernel_precision
        if self._engine is None:
            self._engine = {}
        key = (prec, slot) if not self.low_latency else (prec, slot, "ll")
        eng = self._engine.get(key)
        if eng is None:
            dev = next(self.parameters()).device
            if dev.type != "cuda":
                raise L.FoundDiffHipError("founddiff_amd runs on MI355X only: move the model to a ROCm device "
                                          "(`.to('cuda')`); there is no CPU path")
            eng = self._engine[key] = DAEngine(self.state_dict(), "", dev, prec, low_latency=self.low_latency)
        return eng

    def tower_engine(self, precision=None):
        """A DAEngine(tower_only=True) of this UNet's frozen DA-CLIP encoder in the kernel mode `precision` (default: the sampling
        precision), kept beside the engines of engine(): sample_tiled(condition="slice") runs the tower on whole slices here, so
        that the engines of the tiles keep their tile-sized buffers and their captured graphs.  Same kernels and mode as
        engine().encode_dose, hence the same bits."""
        prec = precision or self.kernel_precision
        if self._engine is None:
            self._engine = {}
        key = (prec, "tower") if not self.low_latency else (prec, "tower", "ll")
        eng = self._engine.get(key)
        if eng is None:
            dev = next(self.parameters()).device
            if dev.type != "cuda":
                raise L.FoundDiffHipError("founddiff_amd runs on MI355X only: move the model to a ROCm device "
                                          "(`.to('cuda')`); there is no CPU path")
            tower = {k: v for k, v in self.state_dict().items() if k.startswith("dose_encoder.")}
            eng = self._engine[key] = DAEngine(tower, "", dev, prec, low_latency=self.low_latency, tower_only=True)
        return eng

    @torch.no_grad()
    def encode_condition(self, x_cond):
        return self.engine().encode_condition(x_cond.contiguous().float())

    @torch.no_grad()
    def forward(self, x, time, x_self_cond=None, reuse_condition=False):
        """x (B,2,H,W) = cat(x_t, x_input) -- (B,3,H,W) with the input_condition plane; time (B,) float.
        Returns (B,1,H,W) fp32."""
        eng = self.engine()
        x = x.float()
        x_t, x_in = x[:, 0:1].contiguous(), x[:, 1:2].contiguous()
        x_c2 = x[:, 2:3].contiguous() if self.input_condition else None
        if not reuse_condition:
            eng.encode_condition(x_in)
        return eng.forward(x_t, x_in, time.float().contiguous(), x_cond2=x_c2).clone()


class UnetRes(nn.Module):
    """reference src/DADiff.py:743-836: one UNet, or two (residual + noise) for the objectives
    'pred_res_noise' / 'pred_x0_noise'."""

    def __init__(self, dim, init_dim=None, out_dim=None, dim_mults=(1, 2, 4, 8), channels=1, self_condition=False,
                 resnet_block_groups=8, learned_variance=False, learned_sinusoidal_cond=False,
                 random_fourier_features=False, learned_sinusoidal_dim=16, num_unet=1, condition=False,
                 input_condition=False, objective="pred_res_noise", test_res_or_noise="res_noise",
                 precision=None, clip_cfg=None):
        super().__init__()
        if num_unet not in (1, 2):
            raise ValueError("num_unet must be 1 or 2")
        self.condition = condition
        self.input_condition = input_condition
        self.channels = channels
        self.out_dim = default(out_dim, channels * (1 if not learned_variance else 2))
        self.random_or_learned_sinusoidal_cond = learned_sinusoidal_cond or random_fourier_features
        self.self_condition = self_condition
        self.num_unet = num_unet
        self.objective = objective
        self.test_res_or_noise = test_res_or_noise
        self.unet0 = Unet(dim, init_dim=init_dim, out_dim=out_dim, dim_mults=dim_mults, channels=channels,
                          self_condition=self_condition, resnet_block_groups=resnet_block_groups,
                          learned_variance=learned_variance, learned_sinusoidal_cond=learned_sinusoidal_cond,
                          random_fourier_features=random_fourier_features,
                          learned_sinusoidal_dim=learned_sinusoidal_dim, condition=condition,
                          input_condition=input_condition, precision=precision, clip_cfg=clip_cfg)
        if num_unet == 2:
            self.unet1 = Unet(dim, init_dim=init_dim, out_dim=out_dim, dim_mults=dim_mults, channels=channels,
                              self_condition=self_condition, resnet_block_groups=resnet_block_groups,
                              learned_variance=learned_variance, learned_sinusoidal_cond=learned_sinusoidal_cond,
                              random_fourier_features=random_fourier_features,
                              learned_sinusoidal_dim=learned_sinusoidal_dim, condition=condition,
                              input_condition=input_condition, precision=precision, clip_cfg=clip_cfg)

    def _unets(self):
        return [self.unet0, self.unet1] if self.num_unet == 2 else [self.unet0]

    def trainable(self):
        """Unet.trainable() of every U-Net of this model: the list of views (one per U-Net).  With two U-Nets this is the
        opt-in to training them: forward, under gradients, then returns both training forwards, and
        ResidualDiffusion.forward / p_losses two losses (Trainer(optimizer='radam') asks for it itself)."""
        return [u.trainable() for u in self._unets()]

    def forward(self, x, time, x_self_cond=None, reuse_condition=False):
        """src/DADiff.py:817-836.  time = [alphas_cumsum[t]*T, betas_cumsum[t]*T].  With gradients enabled on a model whose
        trainable view exists (Unet.trainable(): ResidualDiffusion.forward and Trainer.train ask for it) the call is a training
        forward, Unet.train_forward; under no_grad, and on a model that never trained, it is the engine as ever."""
        unets = self._unets()
        views = [u._trainable is not None for u in unets]
        if torch.is_grad_enabled() and any(views):
            # one training forward per row of the objective (src/DADiff.py:817-823), each behind its own frozen tower
            if self.num_unet == 2 and not all(views):
                raise NotImplementedError("training two U-Nets: the reference optimises them with RAdam, and one of the two has "
                                          "no trainable view: call model.trainable() (DESIGN.md section 8)")
            return [unets[r.unet].train_forward(x, time[r.time]) for r in objectives.routed(self.objective, self.num_unet)]
        kw = dict(x_self_cond=x_self_cond, reuse_condition=reuse_condition)
        if self.num_unet == 2:
            run = objectives.TEST_UNETS.get(self.test_res_or_noise)
            if run is None:
                raise ValueError(f"test_res_or_noise={self.test_res_or_noise!r}")
            return tuple(unets[i](x, time[i], **kw) if i in run else 0 for i in (0, 1))
        return [unets[r.unet](x, time[r.time], **kw) for r in objectives.routed(self.objective, 1)]


class ResidualDiffusion(nn.Module, TiledSampling):
    """Residual (RDDM-style) diffusion sampler, reference src/DADiff.py:908-1380.

    Differences a caller can see: (1) the t-independent DA-CLIP branch is evaluated once per
    `sample()` instead of once per step; (2) `sample/ddim_sample/p_sample_loop/p_sample` take an
    optional `noise=` so that runs are reproducible against a CPU reference (the reference draws
    from the global generator; the default here does too); (3) sample_ensemble and sample_tiled, which the reference does not
    have, are tiled_sampling.TiledSampling's."""
    _normalize, _unnormalize = staticmethod(normalize_to_neg_one_to_one), staticmethod(unnormalize_to_zero_to_one)

    def __init__(self, model, *, image_size, timesteps=1000, sampling_timesteps=None, loss_type="l1",
                 objective="pred_res_noise", ddim_sampling_eta=0., condition=False, sum_scale=None,
                 input_condition=False, input_condition_mask=False, test_res_or_noise="None",
                 use_graph=True, final_fp32_steps=None, ssim_weight=0.0):
        super().__init__()
        # the weight of the structural term of the training loss (diffusion_train.structural_loss; 0.0: none, the reference's
        # loss).  A training setting like loss_type: forward, p_losses and train_step read it, a checkpoint does not hold it
        self.ssim_weight = dt.check_ssim_weight("ResidualDiffusion", ssim_weight)
        assert not (type(self) == ResidualDiffusion and model.channels != model.out_dim)
        assert not model.random_or_learned_sinusoidal_cond
        objectives.check_objective(objective)
        if not condition:
            raise NotImplementedError("condition=True is what the DA-CLIP conditioned Unet supports "
                                      "(it reads x[:,1], src/DADiff.py:692)")
        objectives.check_model(objective, objectives.num_unet(model))
        if timesteps != 1000:
            raise NotImplementedError("init() of the reference hard-codes 1000 timesteps (src/DADiff.py:1034)")
        self.model = model
        self.channels = model.channels
        self.self_condition = model.self_condition
        self.image_size = image_size
        self.objective = objective
        self.condition = condition
        self.input_condition = input_condition
        self.input_condition_mask = input_condition_mask
        self.test_res_or_noise = test_res_or_noise
        self.sum_scale = sum_scale if sum_scale else 0.01
        ddim_sampling_eta = 0.  # forced when condition=True (src/DADiff.py:942)
        self.num_timesteps = int(timesteps)
        self.loss_type = loss_type
        self.sampling_timesteps = default(sampling_timesteps, timesteps)
        assert self.sampling_timesteps <= timesteps
        self.is_ddim_sampling = self.sampling_timesteps < timesteps
        self.ddim_sampling_eta = ddim_sampling_eta
        self.use_graph = use_graph
        # precision schedule of the bf16 mode: the last `final_fp32_steps` UNet forwards of a sampling loop run
        # on the fp32 (parity-mode) engine.  The returned image is clamp(x_input - pred_res) of the LAST forward
        # (src/DADiff.py:1317-1318, 1206), so its rounding error reaches the output undamped while the earlier
        # steps' errors only enter through x_t, weighted by their alpha increments.
        # Default 1: measured at 512x512 / 50 DDIM steps, bf16 alone drifts 1.08e-2 L2 (50.0 dB) from the fp32
        # engine, with the last step in fp32 4.4e-3 (57.8 dB) for +5..7 % time; a second fp32 step buys nothing.
        if final_fp32_steps is None:
            final_fp32_steps = int(os.environ.get("FOUNDDIFF_FINAL_FP32_STEPS", "1"))
        self.final_fp32_steps = int(final_fp32_steps)
        # ... and of that step only the outermost resolution level(s) -- init_conv, downs[0], ups[-1], the final
        # block: 53 % of a forward's bf16 drift originates there (profiles/r02_drift_table.md) at a third of the fp32
        # forward's time -- run one class up, the levels below stay on the fast engine (DAEngine.forward_hybrid).
        # 0: the whole step runs on the higher-precision engine.  Measured at 512x512 / 50 steps against the fp32
        # engine (tools/e2e_drift.py): pure bf16 1.12e-2 L2 / 49.8 dB at 11.0 slices/s; whole last step in fp32
        # 4.6e-3 / 57.5 dB at 10.2; levels 0-1 of the last step in fp32 (default 2) 7.0e-3 / 53.8 dB at 10.5;
        # level 0 alone 1.01e-2 (the error of the inner levels passes through the outer up path undamped).
        # precision='fp16' (the binary16 build of the same kernels): default 0 -- the whole last step on the fp32-storage engine.
        # Its 49 steps leave 1.6e-3 L2 against the CPU oracle at 512x512 (bf16: 1.3e-2); the last step on levels 0-1 makes that
        # 1.06e-3, on all levels 6.3e-4 / 75.6 dB for +2.6 % time (tools/probes/fp16_drift.py; profiles/r06/fp16_mode.md).
        lv = os.environ.get("FOUNDDIFF_FINAL_OUTER_LEVELS")
        self.final_outer_levels = None if lv is None else int(lv)       # (None: the default of the model's precision, see the property)
        self.check_fp16_range = os.environ.get("FOUNDDIFF_FP16_CHECK", "1") != "0"
        # how many of those levels also run their DOWN stage on the tail engine (default: all of them)
        self.final_down_levels = int(os.environ.get("FOUNDDIFF_FINAL_DOWN_LEVELS", "-1"))
        # adaLN vectors of all DDIM steps in one pass in front of the captured loop (DAEngine.time_cond_table) instead of six
        # small launches per step: "auto" = with the one-slice kernel set only (151.4 -> 149.8 ms per 50-step slice at batch 1;
        # in the two-stream throughput mode the small launches of one stream hide under the other's kernels and the table
        # measured -0.3 %: 13.27 vs 13.21 slices/s, alternated); 1 / 0 force it on / off.  Bit for bit the same vectors.
        self._time_table = os.environ.get("FOUNDDIFF_TIME_TABLE", "auto")
        for k, v in residual_schedule(timesteps, after_init=False).items():
            self.register_buffer(k, v)
        self._host_sched = None
        self._slot = 0
        # independent half-batches on concurrent HIP streams: kernels bound by different resources (VALU-issue
        # scan, HBM row-GEMMs, MFMA convolutions) overlap when they come from independent launch sequences
        # (measured: 2 x 8 slices on two streams 1.79 ms per slice-forward, one stream of 8 or 16: 1.90 / 1.84)
        self.streams = int(os.environ.get("FOUNDDIFF_STREAMS", "2"))
        # largest sub-batch one engine is asked to hold (sample() runs bigger batches as consecutive groups): bounds the workspace
        self.max_sub_batch = int(os.environ.get("FOUNDDIFF_MAX_SUB_BATCH", "16"))
        self._side_streams = {}

    def init(self):
        """Re-derive the schedule the way Trainer.test() does before sampling (src/DADiff.py:1033)."""
        dev = self.betas.device
        for k, v in residual_schedule(1000, after_init=True).items():
            setattr(self, k, v.to(dev))
        self.num_timesteps = 1000
        self._host_sched = None
        self._drop_graphs()

    def load_state_dict(self, state_dict, strict=True, assign=False):
        live = {k: v for k, v in state_dict.items() if not any(arch.is_dead_key(k, f"model.{n}.") for n in objectives.UNET_NAMES)}
        return super().load_state_dict(live, strict=strict, assign=assign)     # new weights -> new engines -> new graphs

    # ---- helpers
    def _drop_graphs(self):
        """Forget every captured graph (they bake in scheduler constants): init() re-derives the schedule."""
        for u in objectives.unets_of(self.model):
            for e in (getattr(u, "_engine", None) or {}).values():
                e.graphs.clear()

    def _hs(self):
        if self._host_sched is None:
            self._host_sched = {k: getattr(self, k).detach().cpu() for k in
                                ("alphas_cumsum", "betas_cumsum", "one_minus_alphas_cumsum", "posterior_mean_coef1",
                                 "posterior_mean_coef2", "posterior_mean_coef3", "posterior_log_variance_clipped")}
        return self._host_sched

    def _eng(self):
        return self.model.unet0.engine(slot=self._slot)

    def _unet(self, x_input, x, t_idx, out=None):
        """raw model output for batched integer timesteps t_idx (B,) (src/DADiff.py:1160-1164)"""
        time = (self.alphas_cumsum[t_idx] * self.num_timesteps).float().contiguous()
        return self._eng().forward(x, x_input, time, out=out)

    # ---- objectives other than the shipped one: the rule is objectives.py's, the readings of it are here
    def _plan(self):
        """objectives.SamplePlan -- (mode of fd_res_step_obj, run unet0?, run unet1?, unet0's time entry) -- for this objective /
        test_res_or_noise -- UnetRes.forward (src/DADiff.py:817-836) + model_predictions (1168-1207)."""
        return objectives.sample_plan(self.objective, objectives.num_unet(self.model), self.test_res_or_noise)

    def _is_shipped(self):
        return self._plan() == objectives.SHIPPED_PLAN and not self.input_condition

    def _captured_plan(self):
        """Every plan of _plan() samples on captured loops and device tables unless the model takes a third input plane."""
        return not self.input_condition

    def _obj_loop(self, last, step_noise):
        """Does this call of a plan other than the shipped one run on the captured loops (_obj_ddim / _obj_ancestral)?  The
        eager _generic_loop keeps trajectories (last=False), a step_noise callable and the 3-plane models."""
        return bool(last) and step_noise is None and self._captured_plan() and not self._is_shipped()

    def _group_rows(self):
        """Slices per consecutive group of sample(): streams x max_sub_batch, halved for a plan that runs two engines per stream
        (each then holds max_sub_batch // 2 slices, so a call's workspace stays what max_sub_batch promises) and kept a
        multiple of `streams`."""
        grp = self.streams * self.max_sub_batch
        if self._plan().two_engines:
            grp //= 2
            grp = max(grp - grp % self.streams, self.streams)
        return grp

    def _plan_unets(self):
        """The U-Nets this plan evaluates, unet0 first."""
        return [getattr(self.model, objectives.UNET_NAMES[i]) for i in self._plan().unets]

    def _engines(self):
        """The engines of this plan's U-Nets in the slot of the running sub-batch (slot 0 outside _sample_concurrent)."""
        return [u.engine(slot=self._slot) for u in self._plan_unets()]

    def _o01(self, outs):
        """(o0, o1) as the step kernels (fd_res_step_obj*, fd_tiles_step_*) take them, from the raw outputs of _plan_unets() in
        that order (objectives.SamplePlan.o01)."""
        return self._plan().o01(outs)

    _TIME_CUMSUMS = ("alphas_cumsum", "betas_cumsum")          # the schedule vector behind time input 0 and 1 (times T)

    # ---- the step tables of the captured loops of every plan: pure host functions of the schedule (tests/test_obj_loop_cpu.py)
    def _obj_time_tables(self):
        """(times0, times1): (T,) fp32 CPU tables of the two U-Nets' time inputs, or None where the plan does not run that U-Net --
        entry t is what _outputs feeds at step t."""
        hs, T = self._hs(), self.num_timesteps
        return tuple(None if ti is None else (hs[self._TIME_CUMSUMS[ti]] * T).float().contiguous() for ti in self._plan().times)

    def _obj_anc_table(self):
        """(T, 8) fp32 CPU: row t = {ac, bc, omac, c1, c2, c3, logvar, 0}, the row _par builds for p_sample at step t."""
        hs = self._hs()
        cols = [hs[k].float() for k in ("alphas_cumsum", "betas_cumsum", "one_minus_alphas_cumsum", "posterior_mean_coef1",
                                         "posterior_mean_coef2", "posterior_mean_coef3", "posterior_log_variance_clipped")]
        return torch.stack(cols + [torch.zeros_like(cols[0])], 1).contiguous()

    def _ddim_pairs(self):
        times = list(reversed(torch.linspace(-1, self.num_timesteps - 1, steps=self.sampling_timesteps + 1).int().tolist()))
        return list(zip(times[:-1], times[1:]))

    def _ddim_steps(self):
        """[(time, alpha, last)]: the steps of every DDIM loop -- the timestep, the alpha increment of its update, the last-step flag."""
        acs = self._hs()["alphas_cumsum"]
        return [(time, 0.0 if time_next < 0 else float(acs[time] - acs[time_next]), time_next < 0)
                for time, time_next in self._ddim_pairs()]

    def _obj_ddim_table(self, B):
        """((S, B, 8) parameter rows, (S, B) time inputs of unet0 or None, of unet1 or None), fp32 CPU: step i of the DDIM loop as
        _generic_loop runs it -- {ac, bc, omac, alpha, 0, 0, 0, last} of _par and the time inputs of _outputs."""
        hs = self._hs()
        t0, t1 = self._obj_time_tables()
        steps = self._ddim_steps()
        par = torch.zeros(len(steps), B, 8, dtype=torch.float32)
        for i, (time, alpha, lastf) in enumerate(steps):
            par[i, :, 0], par[i, :, 1], par[i, :, 2] = hs["alphas_cumsum"][time], hs["betas_cumsum"][time], hs["one_minus_alphas_cumsum"][time]
            par[i, :, 3] = alpha
            par[i, :, 7] = float(lastf)
        idx = torch.tensor([t for t, _, _ in steps], dtype=torch.long)
        rows = lambda tab: None if tab is None else tab[idx][:, None].expand(len(steps), B).contiguous()
        return par.contiguous(), rows(t0), rows(t1)

    def _encode_all(self, x_in, cond=None):
        """The conditioning of every engine in use: the tower on x_in, or the preset rows `cond` -- one (prompt_emb, local_all)
        pair per engine of _engines(), row for row the slices of x_in (sample_ensemble)."""
        for i, e in enumerate(self._engines()):
            if cond is None:
                e.encode_condition(x_in)
            else:
                e.load_condition(*cond[i])

    @staticmethod
    def _cond_rows(cond, sl):
        return None if cond is None else [(p[sl], l[sl]) for p, l in cond]

    def _outputs(self, x_in, x, t_idx):
        """raw outputs (o0, o1) of the UNets this configuration evaluates (None where it does not)."""
        plan, T = self._plan(), self.num_timesteps
        c2 = self._xc2 if self.input_condition else None
        times = [(getattr(self, self._TIME_CUMSUMS[plan.times[i]])[t_idx] * T).float().contiguous() for i in plan.unets]
        return (plan.mode,) + plan.o01([u.engine().forward(x, x_in, t, x_cond2=c2).clone() for u, t in zip(self._plan_unets(), times)])

    def _set_cond2(self, x_input_condition):
        """third input plane (src/DADiff.py:1157-1158); already normalised by the caller / sample()."""
        if self.input_condition:
            if not torch.is_tensor(x_input_condition):
                raise ValueError("input_condition=True needs x_input_condition (sample(x_input=[a, b]))")
            self._xc2 = x_input_condition.contiguous().float()

    def _par(self, t_idx, k=(0., 0., 0., 0.), flag=0.):
        B = t_idx.shape[0]
        par = torch.zeros(B, 8, device=t_idx.device, dtype=torch.float32)
        par[:, 0], par[:, 1], par[:, 2] = self.alphas_cumsum[t_idx], self.betas_cumsum[t_idx], self.one_minus_alphas_cumsum[t_idx]
        for i, v in enumerate(k):
            par[:, 3 + i] = v
        par[:, 7] = flag
        return par.contiguous()

    def _step_obj(self, step, x_in, x, t_idx, noise, k=(0., 0., 0., 0.), flag=0., want_preds=False, out=None):
        mode, o0, o1 = self._outputs(x_in, x, t_idx)
        par = self._par(t_idx, k, flag)
        pr = pn = xs = None
        if want_preds:
            pr, pn, xs = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
        else:
            xs = torch.empty_like(x)
        img = (out if out is not None else torch.empty_like(x)) if step else None
        L.call("fd_res_step_obj", mode, step, _p(o0), _p(o1), _p(x), _p(x_in), _p(noise), _p(par), _p(pr), _p(pn),
               _p(xs), _p(img), x.shape[0], x[0].numel(), _stream(x))
        return img, pr, pn, xs

    def predict_noise_from_res(self, x_t, t, x_input, pred_res):
        B = x_t.shape[0]
        pn = torch.empty_like(x_t)
        ac, bc = self.alphas_cumsum[t].contiguous(), self.betas_cumsum[t].contiguous()
        # pred_res is already clamped by the caller; clamp is idempotent
        L.call("fd_res_predictions", _p(pred_res), _p(x_t), _p(x_input), _p(ac), _p(bc), None, _p(pn), None,
               B, x_t[0].numel(), _stream(x_t))
        return pn

    def q_posterior(self, pred_res, x_start, x_t, t):
        """src/DADiff.py:1142-1151.  Small host-side glue over per-batch coefficients."""
        e = lambda a: a[t].reshape(-1, 1, 1, 1)
        mean = torch.empty_like(x_t)
        coef = torch.stack([self.posterior_mean_coef1[t], self.posterior_mean_coef2[t],
                            self.posterior_mean_coef3[t], torch.full_like(self.posterior_mean_coef1[t], -1e30)], 1)
        # mean = c1 x_t + c2 pred_res + c3 x_start, evaluated by the posterior kernel with noise = NULL;
        # the kernel recomputes x_start = clamp(x_in - pred_res); to honour an arbitrary x_start we pass
        # x_in := x_start + pred_res (both already clamped by model_predictions).
        xin_equiv = torch.empty_like(x_t)
        L.call("fd_axpy_f32", _p(x_start.contiguous()), _p(pred_res.contiguous()), 1.0, _p(xin_equiv),
               x_t.numel(), _stream(x_t))
        L.call("fd_res_posterior_step", _p(pred_res.contiguous()), _p(x_t.contiguous()), _p(xin_equiv), None,
               _p(coef.contiguous()), _p(mean), None, x_t.shape[0], x_t[0].numel(), _stream(x_t))
        return mean, e(self.posterior_variance), e(self.posterior_log_variance_clipped)

    @torch.no_grad()
    def model_predictions(self, x_input, x, t, x_input_condition=0, x_self_cond=None, clip_denoised=True,
                          reuse_condition=False):
        """src/DADiff.py:1153-1209."""
        assert clip_denoised, "clip_denoised=False is not built"
        x_input = x_input.contiguous().float()
        x = x.contiguous().float()
        if not self._is_shipped():
            self._set_cond2(x_input_condition)
            if not reuse_condition:
                self._encode_all(x_input)
            _, pr, pn, xs = self._step_obj(0, x_input, x, t, None, want_preds=True)
            return ModelResPrediction(pr, pn, xs)
        if not reuse_condition:
            self._eng().encode_condition(x_input)
        mo = self._unet(x_input, x, t)
        pred_res, pred_noise, x_start = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
        ac, bc = self.alphas_cumsum[t].contiguous(), self.betas_cumsum[t].contiguous()
        L.call("fd_res_predictions", _p(mo), _p(x), _p(x_input), _p(ac), _p(bc), _p(pred_res), _p(pred_noise),
               _p(x_start), x.shape[0], x[0].numel(), _stream(x))
        return ModelResPrediction(pred_res, pred_noise, x_start)

    def p_mean_variance(self, x_input, x, t, x_input_condition=0, x_self_cond=None):
        preds = self.model_predictions(x_input, x, t, x_input_condition, x_self_cond)
        mean, var, logvar = self.q_posterior(preds.pred_res, preds.pred_x_start, x, t)
        return mean, var, logvar, preds.pred_x_start

    @torch.no_grad()
    def p_sample(self, x_input, x, t: int, x_input_condition=0, x_self_cond=None, noise=None,
                 reuse_condition=False, out=None):
        """One ancestral step (src/DADiff.py:1222-1230): UNet forward + fused posterior update."""
        x_input = x_input.contiguous().float()
        x = x.contiguous().float()
        B = x.shape[0]
        hs = self._hs()
        t_idx = torch.full((B,), t, device=x.device, dtype=torch.long)
        if not self._is_shipped():
            if torch.is_tensor(x_input_condition):
                self._set_cond2(x_input_condition)
            if not reuse_condition:
                self._encode_all(x_input)
            if t > 0 and noise is None:
                noise = torch.randn_like(x)
            k = (float(hs["posterior_mean_coef1"][t]), float(hs["posterior_mean_coef2"][t]),
                 float(hs["posterior_mean_coef3"][t]), float(hs["posterior_log_variance_clipped"][t]))
            img, _, _, xs = self._step_obj(2, x_input, x, t_idx, noise if t > 0 else None, k=k, out=out)
            return img, xs
        if not reuse_condition:
            self._eng().encode_condition(x_input)
        mo = self._unet(x_input, x, t_idx)
        coef = torch.tensor([[hs["posterior_mean_coef1"][t], hs["posterior_mean_coef2"][t],
                              hs["posterior_mean_coef3"][t], hs["posterior_log_variance_clipped"][t]]] * B,
                            dtype=torch.float32).to(x.device)
        if t > 0 and noise is None:
            noise = torch.randn_like(x)
        pred_img = out if out is not None else torch.empty_like(x)
        x_start = torch.empty_like(x)
        L.call("fd_res_posterior_step", _p(mo), _p(x), _p(x_input), _p(noise) if t > 0 else None, _p(coef),
               _p(pred_img), _p(x_start), B, x[0].numel(), _stream(x))
        return pred_img, x_start

    @property
    def final_outer_levels(self):
        if self._final_outer_levels is not None:
            return self._final_outer_levels
        return 0 if self.model.unet0.kernel_precision == "fp16" else 2

    @final_outer_levels.setter
    def final_outer_levels(self, v):
        self._final_outer_levels = None if v is None else int(v)

    # ---- the per-step hot loop: graph-captured UNet forward + one scheduler kernel
    def _tail_engine(self, eng):
        """(K, engine or None): the higher-precision engine of the last K steps of a loop (final_fp32_steps):
        fp32 behind the bf16 kernels, bf16 behind the fp8-weight kernels (one precision class up; the fp8 mode is
        the throughput configuration, BASELINE configs[4])."""
        K = self.final_fp32_steps if eng.mode not in ("fp32", "fp32s") else 0
        if K <= 0:
            return 0, None
        # 'fp32s' = fp32 storage with split-bf16 contractions (engine.py): 2^-16 per product is far below the bf16
        # error of the 49 steps before it, at a third of the exact-f32 MFMA's time; FOUNDDIFF_TAIL_EXACT=1 restores 'fp32'
        tail32 = "fp32" if os.environ.get("FOUNDDIFF_TAIL_EXACT") else "fp32s"
        e32 = self.model.unet0.engine(tail32 if eng.mode in ("bf16", "fp16") else "bf16", slot=self._slot)
        e32.share_condition(eng)
        return K, e32

    def _tail_forward(self, e32, eng, img, x_in, time_buf, mo, sched=None):
        """The forward of a tail step: hybrid (outer levels on e32, the rest on eng) or all of it on e32."""
        k = self.final_outer_levels
        if k > 0 and k < len(e32.downs):
            e32.forward_hybrid(eng, img, x_in, time_buf, out=mo, outer_levels=k, sched=sched,
                               down_levels=None if self.final_down_levels < 0 else self.final_down_levels)
        else:
            e32.forward(img, x_in, time_buf, out=mo, sched=sched)

    def _step_forward(self, x_in, img, time_buf, mo, eng=None, tail_of=None):
        eng = eng or self._eng()
        run = (lambda: self._tail_forward(eng, tail_of, img, x_in, time_buf, mo)) if tail_of is not None else \
            (lambda: eng.forward(img, x_in, time_buf, out=mo))
        if not self.use_graph:
            run()
            return
        # captured graphs live and die with the engine whose buffers they bake in
        key = (tuple(img.shape), eng.mode, eng.gen, tail_of.gen if tail_of is not None else 0, self.final_outer_levels, self.final_down_levels)
        bufs = (x_in, img, time_buf, mo)
        g, baked = eng.captured("step", key, run, lambda capture: (capture(run), bufs))
        if [t.data_ptr() for t in baked] != [t.data_ptr() for t in bufs]:
            raise RuntimeError("_step_forward: the step graph of this engine was captured over other buffers than the ones passed "
                               "(x_in, img, time_buf, mo must be the engine's loop buffers, _loop_buffers)")
        g.replay()

    def _loop_buffers(self, x_input, shape):
        eng = self._eng()
        x_in = eng._b("loop_xin", shape, torch.float32)
        x_in.copy_(x_input)
        img = eng._b("loop_img", shape, torch.float32)
        mo = eng._b("model_out", shape, torch.float32)
        time_buf = eng._b("loop_time", (shape[0],), torch.float32)
        return x_in, img, mo, time_buf

    X_T_STEP = 0x7FFFFFFF      # the "step" under which the keyed stream draws x_T (fd_keyed_normal)

    def _slice_seeds(self, slice_seeds, B, dev):
        """(B,) int64 device tensor of per-slice seeds: given, or drawn from torch's global CPU generator (so
        torch.manual_seed makes a run reproducible, like the reference's set_seed)."""
        if slice_seeds is None:
            slice_seeds = torch.randint(0, 2 ** 62, (B,), dtype=torch.int64)
        slice_seeds = torch.as_tensor(slice_seeds, dtype=torch.int64).reshape(-1)
        if slice_seeds.numel() != B:
            raise ValueError(f"slice_seeds must hold one seed per slice ({B}), got {slice_seeds.numel()}")
        return slice_seeds.to(dev).contiguous()

    def _keyed_noise(self, seeds, t, shape):
        nz = torch.empty(shape, device=seeds.device, dtype=torch.float32)
        L.call("fd_keyed_normal", _p(seeds), int(t), _p(nz), shape[0], nz[0].numel(), _stream(nz))
        return nz

    def _noise_and_seeds(self, path, size, dev, noise, slice_seeds, step_noise=None):
        """The one rule for x_T and the per-slice seeds: (noise, seeds) as the sampler behind `path` takes them.  Paths of
        _sample: "group" (the split into consecutive groups), "concurrent", "ddim", "ancestral"; "loop" is p_sample_loop itself.
        Seeds that are not given are one torch.randint on the CPU generator (_slice_seeds), x_T without seeds one torch.randn
        on the device; a None that is returned is drawn by the sampler it goes to."""
        ddim = self.is_ddim_sampling and path != "loop"
        seeds = lambda: self._slice_seeds(slice_seeds, size[0], dev)
        keyed = lambda s: self._keyed_noise(s, self.X_T_STEP, size)
        if path == "ancestral":                                   # p_sample_loop is an entry point of its own: it asks as "loop"
            return noise, slice_seeds
        if path == "group":
            if noise is None:
                noise = torch.randn(size, device=dev) if ddim and slice_seeds is None else keyed(seeds())
            # known oddity: the ancestral sampler without slice_seeds draws them twice, once for x_T above and once for the steps
            return noise, slice_seeds if ddim else seeds()
        if ddim:
            # known inconsistency: "concurrent" ignores slice_seeds while "ddim" and "group" key x_T on them, so a
            # DDIM slice with seeds and no noise depends on its batch size
            if path == "ddim" and noise is None and slice_seeds is not None:
                noise = keyed(seeds())
            return noise, None
        s = seeds() if step_noise is None else None               # "loop", and "concurrent" ancestral (its step noise is keyed)
        if noise is None:
            noise = keyed(s) if s is not None else torch.randn(size, device=dev)
        return noise, s

    def _x_T_into(self, x_in, noise, img):
        """img <- x_T = x_in + sqrt(sum_scale) * noise"""
        L.call("fd_axpy_f32", _p(x_in), _p(noise.contiguous()), math.sqrt(self.sum_scale), _p(img), img.numel(), _stream(img))
        return img

    def _x_T(self, x_in, noise, img):
        """_x_T_into; returns a copy of x_T, the first image of what a loop returns"""
        return self._x_T_into(x_in, noise, img).clone()

    def _finish(self, input_add_noise, img, img_list, last):
        return unnormalize_to_zero_to_one([input_add_noise, img.clone()] if last else [input_add_noise] + img_list)

    @torch.no_grad()
    def p_sample_loop(self, x_input, shape, last=True, noise=None, step_noise=None, slice_seeds=None, _cond=None):
        """src/DADiff.py:1233-1273.  `noise`: the initial randn(shape); `step_noise`: callable t -> tensor (parity
        tests feed the reference's noise this way; one eager step at a time).  Without `step_noise` the step noise is
        the per-slice keyed stream of fd_sched.hip -- a function of (slice_seeds[b], t, pixel) only, so a slice's
        result does not depend on its batch, rank or stream -- and the loop runs from device tables: chunks of steps
        are captured in a HIP graph and replayed (no host work per step).  That holds for every plan of _plan() -- the other
        objectives and the two-U-Net model run _obj_ancestral: fd_obj_begin, one forward per U-Net, fd_res_step_obj_keyed --
        when last=True.  Trajectories (last=False) of those plans, a `step_noise` callable and the 3-plane input_condition
        models run the eager _generic_loop, whose step noise without `step_noise` is torch.randn on the device."""
        if self.input_condition:
            self._set_cond2(x_input[1])
        x_input = x_input[0].contiguous().float()
        if not self._is_shipped():
            if self._obj_loop(last, step_noise):
                noise, seeds = self._noise_and_seeds("loop", shape, x_input.device, noise, slice_seeds)
                return self._obj_ancestral(x_input, shape, noise, seeds, _cond)
            return self._generic_loop(x_input, shape, last, noise, step_noise, ddim=False, cond=_cond)
        x_in, img, mo, time_buf = self._loop_buffers(x_input, shape)
        eng = self._eng()
        self._encode_all(x_in, _cond)
        noise, seeds = self._noise_and_seeds("loop", shape, x_in.device, noise, slice_seeds, step_noise)
        input_add_noise = self._x_T(x_in, noise, img)
        hs = self._hs()
        T = self.num_timesteps
        B = shape[0]
        coefs = torch.stack([hs["posterior_mean_coef1"], hs["posterior_mean_coef2"], hs["posterior_mean_coef3"],
                             hs["posterior_log_variance_clipped"]], 1).float().contiguous().to(x_in.device)      # (T,4)
        times = (hs["alphas_cumsum"] * T).float().contiguous().to(x_in.device)
        img_list = []
        K, e32 = self._tail_engine(eng)
        if seeds is not None:
            self._ancestral_keyed(eng, e32, K, x_in, img, mo, time_buf, coefs, times, seeds, last, img_list)
        else:
            for t in reversed(range(0, T)):
                time_buf.fill_(float(times[t]))
                if t < K:
                    self._step_forward(x_in, img, time_buf, mo, e32, tail_of=eng)
                else:
                    self._step_forward(x_in, img, time_buf, mo, eng)
                coef = coefs[t:t + 1].expand(B, 4).contiguous()
                nz = step_noise(t) if t > 0 else None
                L.call("fd_res_posterior_step", _p(mo), _p(img), _p(x_in), _p(nz), _p(coef), _p(img), None, B,
                       img[0].numel(), _stream(img))
                if not last:
                    img_list.append(img.clone())
        return self._finish(input_add_noise, img, img_list, last)

    def _ancestral_keyed(self, eng, e32, K, x_in, img, mo, time_buf, coefs, times, seeds, last, img_list):
        """The T ancestral steps with the timestep in a device counter: fd_ancestral_begin (t <- t - 1, UNet time
        input) -> UNet forward -> fd_res_posterior_step_keyed (coefficient row t, keyed noise).  With last=True the
        T - K main steps run as replays of one captured chunk of G steps and the K tail steps (higher-precision
        engine) as a second graph."""
        T, B = self.num_timesteps, x_in.shape[0]
        npix = img[0].numel()
        t_dev = eng._b("loop_t", (1,), torch.int32)
        t_dev.fill_(T)
        # graphs bake the pointers of coefs / times / seeds: keep them in engine-owned buffers
        gco, gti, gse = eng._b("loop_coefs", tuple(coefs.shape), torch.float32), eng._b("loop_times", (T,), torch.float32), \
            eng._b("loop_seeds", (B,), torch.int64)
        gco.copy_(coefs)
        gti.copy_(times)
        gse.copy_(seeds)

        def one(e):
            L.call("fd_ancestral_begin", _p(t_dev), _p(gti), _p(time_buf), B, _stream(img))
            if e is eng:
                e.forward(img, x_in, time_buf, out=mo)
            else:
                self._tail_forward(e, eng, img, x_in, time_buf, mo)
            L.call("fd_res_posterior_step_keyed", _p(mo), _p(img), _p(x_in), _p(gco), _p(t_dev), _p(gse), _p(img), None,
                   B, npix, _stream(img))

        K = max(0, min(int(K), T))                                # a tail longer than the loop is the whole loop
        key = lambda G: (tuple(img.shape), eng.mode, eng.gen, G, K, e32.gen if e32 else 0, self.final_outer_levels,
                         self.final_down_levels, T)

        def warm():
            eng.forward(img, x_in, time_buf, out=mo)
            if e32 is not None:
                self._tail_forward(e32, eng, img, x_in, time_buf, mo)
        self._anc_run(eng, "anc", key, warm, lambda: one(eng), img, t_dev, T - K, tail=lambda: one(e32), K=K,
                      graph=self.use_graph and last, each=None if last else lambda: img_list.append(img.clone()))

    def _anc_chunks(self, n):
        """(G, reps, rem): n ancestral steps as `rem` single steps in front of `reps` chunks of G.  G is the largest divisor of n
        in [8, 64]; when there is none (n prime or small) a fixed 40, with n % 40 single steps.  _anc_max_chunks (bench.py's
        bounded leg: time a few chunks, not the volume) keeps at most that many chunks and no single step."""
        G = max([g for g in range(8, 65) if n > 0 and n % g == 0] or [40])
        reps, rem = n // G, n % G
        lim = getattr(self, "_anc_max_chunks", None)
        if lim:
            reps, rem = min(reps, int(lim)), 0
        return G, reps, rem

    @staticmethod
    def _keeping(do, *state):
        """do() with the tensors `state` as they were before it: a capture does not execute, and what it records must not be
        left half-applied -- x_T, and the step counter of the ancestral loops, are put back."""
        saved = [t.clone() for t in state]
        res = do()
        for t, t0 in zip(state, saved):
            t.copy_(t0)
        return res

    def _anc_run(self, own, kind, key, warm, step, img, t_dev, n, tail=None, K=0, graph=True, each=None):
        """The chunked ancestral loop of every plan: n main steps `step()` (_anc_chunks: single steps, then chunks of G) and K tail
        steps `tail()`, the step counter t_dev running down on the device.  graph: a chunk is ONE graph of `own` under `kind` and
        key(G), replayed; the K tail steps are a second graph of the same entry.  Otherwise every step runs eagerly, `each()` after
        it.  Where _anc_max_chunks cut main steps off, the counter jumps to the tail.  Writes _anc_steps_run."""
        G, reps, rem = self._anc_chunks(n)
        done = rem + reps * G

        def run(fn, count):
            for _ in range(count):
                fn()
                if each is not None:
                    each()
        chunk, tail_k = (lambda: run(step, G)), (lambda: run(tail, K))
        if graph and (reps > 0 or K > 0):
            gm, gt = own.captured(kind, key(G), warm, lambda capture: self._keeping(
                lambda: (capture(chunk) if reps > 0 else None, capture(tail_k) if K > 0 else None), img, t_dev))
            chunk, tail_k = gm.replay if reps > 0 else None, gt.replay if K > 0 else None
        run(step, rem)
        for _ in range(reps):
            chunk()
        if K > 0:
            if done < n:
                t_dev.fill_(K)                                    # jump to the tail steps
            tail_k()
        self._anc_steps_run = done + K

    @property
    def time_table(self):
        if self._time_table in ("0", "1"):
            return self._time_table == "1"
        return bool(getattr(self._eng(), "low_latency", False))

    @torch.no_grad()
    def ddim_sample(self, x_input, shape, last=True, noise=None, _cond=None):
        """src/DADiff.py:1276-1365 (eta = 0, type 'use_pred_noise')."""
        if self.input_condition:
            self._set_cond2(x_input[1])
        x_input = x_input[0].contiguous().float()
        if not self._is_shipped():
            if self._obj_loop(last, None):
                return self._obj_ddim(x_input, shape, noise, _cond)
            return self._generic_loop(x_input, shape, last, noise, None, ddim=True, cond=_cond)
        x_in, img, mo, time_buf = self._loop_buffers(x_input, shape)
        eng = self._eng()
        self._encode_all(x_in, _cond)
        T, S = self.num_timesteps, self.sampling_timesteps
        steps = self._ddim_steps()
        if noise is None:
            noise = torch.randn(shape, device=x_in.device)
        input_add_noise = self._x_T(x_in, noise, img)
        hs = self._hs()
        acs = hs["alphas_cumsum"]
        img_list = []

        K, e32 = self._tail_engine(eng)

        def run_steps(forward, fold=False):
            """fold: the forward applies the DDIM update itself (DAEngine.forward sched=: in the bf16 mode inside the
            epilogue of its last kernel), with the step's constants baked into the captured loop graph; the adaLN vectors
            of all steps come from ONE pass in front of the loop (DAEngine.time_cond_table) instead of six small launches
            per step."""
            if fold and self.time_table:
                eng.time_cond_table()
            for i, (time, alpha, lastf) in enumerate(steps):
                if fold and self.time_table and i < S - K:
                    forward(eng, (alpha, lastf), i)
                    continue
                time_buf.fill_(float(acs[time] * T))
                if fold:
                    forward(e32 if i >= S - K else eng, (alpha, lastf))
                    continue
                forward(e32 if i >= S - K else eng)
                L.call("fd_res_ddim_step", _p(mo), _p(img), _p(x_in), None, alpha, 0.0, int(lastf), _p(img),
                       img.numel(), _stream(img))
                if not last:
                    img_list.append(img.clone())

        if self.use_graph and last and os.environ.get("FOUNDDIFF_LOOP_GRAPH", "1") != "0":
            # the whole S-step loop as ONE HIP graph (S x (time fill + 141 kernels + DDIM update), every
            # scheduler constant baked into its node): replayed per sample() on the persistent loop buffers
            key = (tuple(shape), eng.mode, eng.gen, S, T, K, e32.gen if e32 else 0, self.final_outer_levels, self.final_down_levels,
                   self.time_table)

            def fwd(e, sched=None, step=None):
                if e is eng:
                    e.forward(img, x_in, time_buf, out=mo, sched=sched, step=step)
                else:
                    self._tail_forward(e, eng, img, x_in, time_buf, mo, sched=sched)

            def warm():
                if self.time_table:                                # (host -> device copy and buffers: before the capture)
                    eng.time_table_prepare([acs[t] * T for t, _, _ in steps], shape[0])
                    eng.time_cond_table()
                for e in (eng, e32):
                    if e is not None:
                        fwd(e)

            record = lambda capture: self._keeping(lambda: capture(lambda: run_steps(fwd, fold=True)), img)
            eng.captured("ddim_loop", key, warm, record).replay()
        else:
            run_steps(lambda e: self._step_forward(x_in, img, time_buf, mo, e, tail_of=None if e is eng else eng))
        return self._finish(input_add_noise, img, img_list, last)

    # ---- the captured loops of every plan other than the shipped one
    def _obj_buffers(self, x_input, shape, cond):
        """The persistent loop buffers of this plan on the engines of the running slot, x_in loaded and the conditioning of every
        engine in place: (engines, mode, x_in, img, (o0, o1) as the step kernels take them, [(engine, time buffer, output buffer)
        of unet0, the same of unet1]) -- (None, None, None) where the plan does not run that U-Net."""
        plan = self._plan()
        engines = self._engines()
        own = engines[0]                                          # holds what the U-Nets share, and the loop's graph
        x_in = own._b("obj_xin", shape, torch.float32)
        x_in.copy_(x_input)
        img = own._b("obj_img", shape, torch.float32)
        self._encode_all(x_in, cond)
        nets = [(e, e._b("obj_time", (shape[0],), torch.float32), e._b("obj_out", shape, torch.float32)) if e else (None, None, None)
                for e in (engines[0] if plan.run0 else None, engines[-1] if plan.run1 else None)]
        return engines, plan.mode, x_in, img, plan.o01([out for _, _, out in nets if out is not None]), nets

    def _obj_key(self, engines, shape):
        return (tuple(shape), self._plan(), self.num_timesteps) + tuple((e.mode, e.gen) for e in engines)

    def _obj_ddim(self, x_input, shape, noise, cond=None):
        """ddim_sample(last=True) of a plan other than the shipped one: per step one forward per U-Net of the plan, one after the
        other on the same stream, into its own output buffer, and fd_res_step_obj(step = 1) in place on img; the S x B parameter
        rows and time inputs are uploaded before the loop.  use_graph: the whole loop is ONE graph of the plan's first engine
        (kind "obj_ddim"); otherwise the same launches run eagerly -- the same bits, and those of _generic_loop's last image."""
        engines, mode, x_in, img, (o0, o1), nets = self._obj_buffers(x_input, shape, cond)
        own = engines[0]
        B, S = shape[0], self.sampling_timesteps
        npix = img[0].numel()
        par, tt0, tt1 = self._obj_ddim_table(B)
        gpar = own._b("obj_ddim_par", (S, B, 8), torch.float32)
        gpar.copy_(par)
        tabs = []
        for (e, _, out), tt in zip(nets, (tt0, tt1)):
            if e is not None:
                gt = e._b("obj_ddim_time", (S, B), torch.float32)
                gt.copy_(tt)
                tabs.append((e, gt, out))
        if noise is None:
            noise = torch.randn(shape, device=x_in.device)
        input_add_noise = self._x_T(x_in, noise, img)

        def forwards(i):
            for e, gt, out in tabs:
                e.forward(img, x_in, gt[i], out=out)

        def run():
            for i in range(S):
                forwards(i)
                L.call("fd_res_step_obj", mode, 1, _p(o0), _p(o1), _p(img), _p(x_in), None, _p(gpar[i]), None, None, None,
                       _p(img), B, npix, _stream(img))

        if self.use_graph:
            own.captured("obj_ddim", self._obj_key(engines, shape) + (S,), lambda: forwards(0),
                         lambda capture: self._keeping(lambda: capture(run), img)).replay()
        else:
            run()
        return self._finish(input_add_noise, img, [], True)

    def _obj_ancestral(self, x_input, shape, noise, seeds, cond=None):
        """p_sample_loop(last=True) of a plan other than the shipped one, step noise keyed by `seeds`: T steps of fd_obj_begin
        (t <- t - 1 on the device, both time inputs) -> one forward per U-Net of the plan, one after the other on the same stream
        -> fd_res_step_obj_keyed (row t of the (T, 8) table, keyed noise, in place on img).  use_graph: replays of one captured
        chunk of G steps (kind "obj_anc", _anc_run); otherwise the same three launches eagerly, one step at a time -- the same
        bits.  There is no precision tail: _anc_max_chunks simply stops after that many chunks."""
        engines, mode, x_in, img, (o0, o1), nets = self._obj_buffers(x_input, shape, cond)
        own = engines[0]
        T, B = self.num_timesteps, shape[0]
        npix = img[0].numel()
        t_dev = own._b("obj_t", (1,), torch.int32)
        gpar, gse = own._b("obj_anc_par", (T, 8), torch.float32), own._b("obj_seeds", (B,), torch.int64)
        gpar.copy_(self._obj_anc_table())
        gse.copy_(seeds)
        gts = [None, None]
        for i, ((e, tb, _), tt) in enumerate(zip(nets, self._obj_time_tables())):
            if e is not None:
                gts[i] = e._b("obj_anc_time", (T,), torch.float32)
                gts[i].copy_(tt)
                tb.zero_()
        (_, tb0, _), (_, tb1, _) = nets
        input_add_noise = self._x_T(x_in, noise, img)
        t_dev.fill_(T)

        def forwards():
            for e, tb, out in nets:
                if e is not None:
                    e.forward(img, x_in, tb, out=out)

        def one():
            L.call("fd_obj_begin", _p(t_dev), _p(gts[0]), _p(gts[1]), _p(tb0), _p(tb1), B, T, _stream(img))
            forwards()
            L.call("fd_res_step_obj_keyed", mode, _p(o0), _p(o1), _p(img), _p(x_in), _p(gpar), _p(t_dev), _p(gse), _p(img),
                   B, npix, T, _stream(img))
        self._anc_run(own, "obj_anc", lambda G: self._obj_key(engines, shape) + (G,), forwards, one, img, t_dev, T,
                      graph=self.use_graph)
        return self._finish(input_add_noise, img, [], True)

    def _generic_loop(self, x_in, shape, last, noise, step_noise, ddim, cond=None):
        """The eager form of p_sample_loop / ddim_sample for the plans other than the shipped one: eager UNet forwards (one or two
        per step, slot 0's engines) + one fd_res_step_obj launch per step, torch.randn step noise unless `step_noise` gives it.
        It serves what the captured loops (_obj_ddim / _obj_ancestral) do not: trajectories (last=False), a step_noise callable
        (the parity tests feed the reference's noise this way) and the 3-plane input_condition models."""
        self._encode_all(x_in, cond)
        B = shape[0]
        if noise is None:
            noise = torch.randn(shape, device=x_in.device)
        img = torch.empty_like(x_in)
        input_add_noise = self._x_T(x_in, noise, img)
        img_list = []
        if ddim:
            for time, alpha, lastf in self._ddim_steps():
                t_idx = torch.full((B,), time, device=x_in.device, dtype=torch.long)
                img = self._step_obj(1, x_in, img, t_idx, None, k=(alpha, 0., 0., 0.), flag=float(lastf))[0]
                if not last:
                    img_list.append(img.clone())
        else:
            for t in reversed(range(0, self.num_timesteps)):
                nz = None
                if t > 0:
                    nz = step_noise(t) if step_noise is not None else torch.randn(shape, device=x_in.device)
                img, _ = self.p_sample(x_in, img, t, noise=nz, reuse_condition=True)
                if not last:
                    img_list.append(img.clone())
        return self._finish(input_add_noise, img, img_list, last)

    @torch.no_grad()
    def sample(self, x_input=0, batch_size=16, last=True, noise=None, step_noise=None, slice_seeds=None):
        """src/DADiff.py:1368-1380: x_input = [ldct (B,1,H,W) in [0,1]] -> list of images in ~[0,1].
        `slice_seeds` (B int64): per-slice keys of the ancestral sampler's step noise (and of x_T when `noise` is not
        given) -- see p_sample_loop; founddiff_amd.parallel.sample_volume passes seed + GLOBAL slice index."""
        x_input = list(x_input)
        return self._range_checked(lambda: self._sample(x_input, batch_size, last, noise, step_noise, slice_seeds),
                                   "the sampled image", image=lambda res: res[-1])

    def _range_checked(self, run, what, image=lambda res: res):
        """run(), under the range check of the 'fp16' kernels.  binary16 ends at 65504: an activation beyond it is stored as
        infinity and reaches the image as NaN (the clamps of the scheduler kernels propagate NaN like torch.clamp).  One reduction
        + one host read of image(what run returned) per call: precision='fp16' raises, 'auto' moves the model to the bfloat16
        kernels for good and runs once more."""
        res = run()
        if self.model.unet0.kernel_precision == "fp16" and self.check_fp16_range and not bool(torch.isfinite(image(res)).all()):
            if self.model.unet0.precision != "auto":
                raise L.FoundDiffHipError(
                    f"precision='fp16': {what} is not finite -- an activation of this checkpoint "
                    "left IEEE binary16's range (65504).  Use precision='bf16' (same speed, fp32's range, 8 significand bits), "
                    "'auto' or 'fp32s'.")
            import warnings
            warnings.warn("founddiff_amd: precision='auto': this checkpoint's activations leave IEEE binary16's range; "
                          "this and every later sample() of the model run on the bfloat16 kernels")
            for u in objectives.unets_of(self.model):
                u._auto_bf16 = True
            res = run()
        return res

    def _sample(self, x_input, batch_size, last, noise, step_noise, slice_seeds, cond=None):
        """`cond`: the preset conditioning of sample_ensemble (_encode_all), whose x_input is already in [-1, 1]; it is sliced the
        way `noise` is and no tower runs."""
        x_input = list(x_input)
        # Workspace bound: an engine's workspace grows with its sub-batch (~1.9 GB per 512x512 slice in bf16,
        # twice that in the fp32 modes) and a sample() keeps `streams` engines plus their tail engines alive.  Batches beyond
        # streams x max_sub_batch slices run as consecutive groups of that size on the same engines: a slice's result does not
        # depend on its batch, so the output is the same bits; the workspace stays that of one group whatever the batch.
        # A plan with two engines per stream halves the group (_group_rows): each engine then holds max_sub_batch // 2 slices.
        grp = self._group_rows()
        if (self._captured_plan() and last and step_noise is None and x_input[0].shape[0] > grp
                and x_input[0].shape[0] % self.streams == 0):
            dev = x_input[0].device
            batch_size = x_input[0].shape[0]
            size = tuple(x_input[0].shape)
            noise, slice_seeds = self._noise_and_seeds("group", size, dev, noise, slice_seeds)
            x01 = x_input[0]                             # (still the caller's [0, 1] tensor: the groups normalise their own slices)
            parts = []
            for g0 in range(0, batch_size, grp):
                sl = slice(g0, min(g0 + grp, batch_size))
                parts.append(self._sample([x01[sl]], sl.stop - sl.start, True, noise[sl].contiguous(), None,
                                          None if slice_seeds is None else slice_seeds[sl], self._cond_rows(cond, sl)))
            return [torch.cat([p[j] for p in parts], 0) for j in range(len(parts[0]))]
        if self.input_condition and self.input_condition_mask:     # src/DADiff.py:1372-1375
            x_input[0] = normalize_to_neg_one_to_one(x_input[0])
        elif cond is None:
            x_input = normalize_to_neg_one_to_one(x_input)
        batch_size, channels, h, w = x_input[0].shape
        size = (batch_size, channels, h, w)
        # two concurrent sub-batches: DDIM, and the ancestral sampler when its step noise is the keyed stream
        # (a two-engine plan also goes there with fewer than 8 slices when one engine could not hold them within its half of
        # max_sub_batch: the groups of a split of such a plan are that small when max_sub_batch is)
        big = batch_size >= 8 or (self._group_rows() < self.streams * self.max_sub_batch and batch_size > self.max_sub_batch // 2)
        nsl = self.streams if (self._captured_plan() and last and big and batch_size % self.streams == 0 and
                               (self.is_ddim_sampling or step_noise is None)) else 1
        path = "concurrent" if nsl > 1 else "ddim" if self.is_ddim_sampling else "ancestral"
        noise, seeds = self._noise_and_seeds(path, size, x_input[0].device, noise, slice_seeds)
        pre = {} if cond is None else {"_cond": cond}              # (absent without a preset: the calls are today's)
        if nsl > 1:
            return self._sample_concurrent(x_input[0], size, noise, nsl, seeds, **pre)
        if self.is_ddim_sampling:
            return self.ddim_sample(x_input, size, last=last, noise=noise, **pre)
        return self.p_sample_loop(x_input, size, last=last, noise=noise, step_noise=step_noise, slice_seeds=seeds, **pre)

    def _sample_concurrent(self, x_in, size, noise, nsl, seeds=None, _cond=None):
        """Sampling of a batch (DDIM; ancestral with keyed step noise: `seeds`) as `nsl` independent sub-batches, each on its own HIP stream with its own engine
        (workspaces, captured loop graph).  A slice's result does not depend on what else is in its batch (kernel
        configurations depend on the image size only), so the output is bit-identical to the single-stream run."""
        B = size[0]
        per = B // nsl
        main = torch.cuda.current_stream(x_in.device)
        if noise is None:
            noise = torch.randn(size, device=x_in.device)
        outs = []
        for k in range(nsl):
            st = self._side_streams.get(k)
            if st is None:
                st = self._side_streams[k] = torch.cuda.Stream(device=x_in.device)
            st.wait_stream(main)
            self._slot = k
            try:
                with torch.cuda.stream(st):
                    sl = slice(k * per, (k + 1) * per)
                    if seeds is None:
                        o = self.ddim_sample([x_in[sl].contiguous()], (per,) + tuple(size[1:]), last=True,
                                             noise=noise[sl].contiguous(), _cond=self._cond_rows(_cond, sl))
                    else:
                        o = self.p_sample_loop([x_in[sl].contiguous()], (per,) + tuple(size[1:]), last=True,
                                               noise=noise[sl].contiguous(), slice_seeds=seeds[sl], _cond=self._cond_rows(_cond, sl))
            finally:
                self._slot = 0
            outs.append((st, o))
        for st, o in outs:
            main.wait_stream(st)
            for t in o:
                t.record_stream(main)
        return [torch.cat([o[j] for _, o in outs], 0) for j in range(len(outs[0][1]))]

    # ---- training (src/DADiff.py:1382-1499)
    def weights_changed(self):
        """The parameters were written in place (ClipAdamEMA's raw pointers): forget the captured graphs and the packed engines."""
        self._drop_graphs()
        for u in objectives.unets_of(self.model):
            u.weights_changed()

    def clone(self):
        """A deep copy with its own parameters and no engines, graphs or streams (the EMA model of Trainer.train)."""
        self.weights_changed()
        unets = objectives.unets_of(self.model)
        saved, self._side_streams = self._side_streams, {}
        engines = [u._train_engine for u in unets]
        for u in unets:
            u._train_engine = None
        try:
            return copy.deepcopy(self)
        finally:
            self._side_streams = saved
            for u, e in zip(unets, engines):
                u._train_engine = e

    def _train_ready(self, fn):
        if objectives.num_unet(self.model) != 1:
            # opt-in: the raising default is pinned by tests
            if any(u._trainable is None for u in objectives.unets_of(self.model)):
                raise NotImplementedError(f"{fn}: training two U-Nets: the reference optimises them with RAdam, and this is opt-in: "
                                          "call model.trainable() on the UnetRes first, or train through Trainer(optimizer=\"radam\") "
                                          f"(DESIGN.md section 8); objectives {objectives.ONE_UNET_TEXT} train one")
            return
        self.model.unet0.trainable()

    def p_losses(self, imgs, t, noise=None, slice_seeds=None, step=0, scale=1.0):
        """diffusion_train.p_losses (src/DADiff.py:1399-1482) on this class: imgs = [x_start, x_input] already normalised.  Asks
        for the trainable view first, so that a bare call on a fresh model is a training forward and not the no_grad engine."""
        self._train_ready("ResidualDiffusion.p_losses")
        return dt.p_losses(self, imgs, t, noise, slice_seeds, step, scale)

    def forward(self, imgs, t=None, noise=None, slice_seeds=None, step=0):
        """src/DADiff.py:1382-1397: imgs = [x_start, x_input], (B, 1, H, W) in [0, 1], or a diffusion_train.StoreBatch -> the list
        of losses (one U-Net: one), differentiable in the trunk's parameters.  t (B,) int64 is drawn as the reference draws it unless given; noise, or
        slice_seeds (+ step) for the keyed per-slice stream, as diffusion_train.q_sample takes them.  RuntimeError for CPU tensors
        (there is no CPU path).  Two U-Nets ('pred_res_noise', 'pred_x0_noise') give two losses once model.trainable() was called
        (Trainer(optimizer='radam') does), NotImplementedError before that."""
        fn = "ResidualDiffusion.forward"
        self._train_ready(fn)
        model_fn, schedule, objective, loss_type, ssim_weight = dt._diffusion_args(fn, self)
        if isinstance(imgs, dt.StoreBatch):
            if t is None:
                t = torch.randint(0, self.num_timesteps, (len(imgs),), device=imgs.device).long()
        elif not isinstance(imgs, (list, tuple)) or len(imgs) != 2 or not all(isinstance(v, torch.Tensor) for v in imgs):
            raise RuntimeError(f"{fn}: imgs must be [x_start, x_input] (condition=True without an input condition)")
        elif t is None:
            t = torch.randint(0, self.num_timesteps, (imgs[0].shape[0],), device=imgs[0].device).long()
        return dt.p_losses_fn(model_fn, imgs, t, schedule, objective, loss_type, noise, slice_seeds, step, 1.0, normalize=True,
                              ssim_weight=ssim_weight)

    @torch.no_grad()
    def eval_items(self, imgs, t, noise=None, slice_seeds=None, step=0, precision="fp32", ssim=False):
        """What forward() measures, per slice and forward-only: imgs, t, noise, slice_seeds and step as forward takes them (t is
        required) -> one (B, 2) device tensor per U-Net the objective trains, diffusion_train.val_items of its output: column 0
        the slice's loss against p_losses' target (the mean over the batch is forward()'s loss), column 1 the one-step
        denoising error clamp(x_input - clamp(pred_res)) against x_start in [0, 1] units where the output is a residual
        ('pred_res', and unet0 of 'pred_res_noise'), NaN elsewhere.  q_sample, then per U-Net its inference engine:
        encode_condition, forward, val_items; unet0 gets times[0] (times[1] for 'pred_noise'), unet1 times[1].  Nothing asks for
        the trainable view or touches requires_grad, so this runs on a model that never trained, on the EMA copy and on two
        U-Nets.  precision: the engine's; 'fp32' by default, the precision training runs in, None for the model's sampling
        precision.  The engines hold packed weights: after an optimiser step, weights_changed() comes first.
        ssim=True: every tensor is (B, 3); column 2 is the SSIM of that one-step estimate by the definition Trainer.test reports
        (metrics.compute_metrics, clamped map) on the pair diffusion_train.onestep_pair writes, NaN where column 1 is."""
        fn = "ResidualDiffusion.eval_items"
        _, schedule, objective, loss_type, _ = dt._diffusion_args(fn, self)
        x_in, times, targets = dt._diffused(fn, imgs, t, schedule, noise, slice_seeds, step, True, x0_out=True)
        x_t, x_input = x_in[:, 0:1].contiguous(), x_in[:, 1:2].contiguous()
        out = []
        with torch.cuda.device(x_in.device):
            for r in objectives.TRAINING[objective]:              # UnetRes.forward's routing, p_losses_fn's targets
                eng = getattr(self.model, objectives.UNET_NAMES[r.unet]).engine(precision)
                eng.encode_condition(x_input)
                pred = eng.forward(x_t, x_input, times[r.time])
                items = dt.val_items(pred, targets[r.target], loss_type, *((x_input, targets["x0"]) if r.residual else ()))
                if ssim:
                    if r.residual:
                        from .metrics import compute_metrics
                        col = compute_metrics(*dt.onestep_pair(pred, x_input, targets["x0"]))[:, 1:2]
                    else:
                        col = torch.full_like(items[:, :1], float("nan"))
                    items = torch.cat([items, col], 1)
                out.append(items)
        return out
