"""The reference Trainer's surface (src/DADiff.py:1506-1966) around this project's samplers and training step: `Trainer` with
`train`, `save`, `load`, `validate`, `sample` and `test`, and the stand-ins `_Accel` and `_EMAView` for what the reference takes from
accelerate and ema_pytorch.  `founddiff_amd.DADiff` re-exports every name, so `from founddiff_amd.DADiff import Trainer` reads as the
reference's.  The Trainer drives a diffusion model through its methods alone (sample, sample_ensemble, sample_tiled, eval_items,
clone, weights_changed, init) and never names the ResidualDiffusion class: this module does not import DADiff.py and launches
nothing itself."""
import math
import os
from collections import namedtuple

import numpy as np
import torch

from . import diffusion_train as dt
from . import objectives
from .ensemble import (ORIENTATIONS_D4, ORIENTATIONS_FLIPS, IntervalCalibration, interval_grid, quantile_suffix, quantile_table,
                       risk_control)
from .metrics import INTERVAL_FLOOR, check_interval_grid, interval_coverage, interval_hist, interval_scale
from .schedule import load_weights
from .tiling import tiled_ensemble_opt_in

# Trainer.test's quantiles: the levels handed to sample_ensemble, the caller's among them (the first ones), the index of the
# estimate's level or None
_QuantilePlan = namedtuple("_QuantilePlan", ["levels", "user", "estimate"])
_IntervalPlan = namedtuple("_IntervalPlan", ["scale", "floor", "nominal"])        # nominal: 1 - alpha of a calibration, or None


def _ensemble_plan(fn, n_samples, quantiles, estimate, tile, tiled_ensemble, orientations):
    """The argument checks that `fn` (Trainer.test, Trainer.calibrate_intervals) makes before any sampling, and the _QuantilePlan
    of the call (None without levels): the levels sample_ensemble is asked for, the caller's, and the place of the 0.5 level
    under estimate="median"."""
    if orientations is not None and tile is not None:
        raise RuntimeError(f"{fn}: orientation ensembles of tiled samples are not built")
    if int(n_samples) < 1:
        raise RuntimeError(f"{fn}: n_samples must be at least 1 (got {n_samples})")
    if estimate not in ("mean", "median"):
        raise RuntimeError(f"{fn}: estimate must be 'mean' or 'median' (got {estimate!r})")
    if (quantiles is not None or estimate == "median") and int(n_samples) <= 1:
        raise RuntimeError(f"{fn}: quantiles and estimate='median' need an ensemble, n_samples > 1 (got {n_samples})")
    qplan = None
    if quantiles is not None or estimate == "median":
        levels = tuple(float(q) for q in (() if quantiles is None else quantiles))
        n_user = len(levels)
        if estimate == "median" and 0.5 not in levels:
            levels = levels + (0.5,)
        quantile_table(levels, int(n_samples))
        quantile_suffix(levels[:n_user])
        qplan = _QuantilePlan(levels, levels[:n_user], levels.index(0.5) if estimate == "median" else None)
    tiled_ensemble_opt_in(fn, tile, n_samples, tiled_ensemble)
    return qplan


def _interval_settings(model, n_samples, levels, estimate, floor, tile, overlap, tile_condition, tile_fuse, orientations):
    """What a calibrated scale is valid for, as JSON holds it: the ensemble, the interval, the sampler and the model's objective.
    `model`: the diffusion model that samples (None in a check that has none: its fields are then None)."""
    from .tiling import tile_pair
    if orientations is None:
        codes = None
    elif isinstance(orientations, str):                                  # the named sets as their codes: "flips" is (0, 1, 2, 3)
        codes = list({"d4": ORIENTATIONS_D4, "flips": ORIENTATIONS_FLIPS}.get(orientations, ())) or orientations
    else:
        codes = [int(c) for c in orientations]
    steps = getattr(model, "sampling_timesteps", None)
    return {
        "n_samples": int(n_samples), "levels": [float(q) for q in levels], "estimate": estimate,
        "floor": None if floor is None else float(floor),
        "sampler": None if model is None else ("ddim" if getattr(model, "is_ddim_sampling", False) else "ancestral"),
        "sampling_timesteps": None if steps is None else int(steps),
        "objective": getattr(model, "objective", None),
        "tile": None if tile is None else [int(v) for v in tile_pair("Trainer", tile, "tile")], "overlap": int(overlap) if tile is not None else 0,
        "tile_condition": tile_condition if tile is not None else None, "tile_fuse": tile_fuse if tile is not None else None,
        "orientations": codes,
    }


class _Accel:
    """Stand-in for the accelerate attributes train.py reads (train.py:162-177)."""
    is_local_main_process = True
    is_main_process = True

    def __init__(self, device, group=None, data_parallel=False):
        """data_parallel: the attributes become those of this rank of `group` (Trainer(data_parallel=True))"""
        self.device, self.group, self.data_parallel = device, group, bool(data_parallel)
        if self.data_parallel:
            import torch.distributed as dist
            self.is_main_process = dist.get_rank(group) == 0
            self.is_local_main_process = int(os.environ.get("LOCAL_RANK", dist.get_rank(group))) == 0

    def wait_for_everyone(self):
        if self.data_parallel:
            import torch.distributed as dist
            if dist.get_backend(self.group) == "nccl" and self.device.index is not None:
                dist.barrier(group=self.group, device_ids=[self.device.index])
            else:
                dist.barrier(group=self.group)


class _EMAView:
    """`trainer.ema.ema_model` of the reference (ema_pytorch wrapper around the diffusion)."""

    def __init__(self, model):
        self.ema_model = model

    def to(self, device):
        self.ema_model.to(device)
        return self

    def load_state_dict(self, sd, strict=True):
        live = {k[len("ema_model."):]: v for k, v in sd.items() if k.startswith("ema_model.")}
        if strict:
            return load_weights(self.ema_model, live, "ema state")
        return self.ema_model.load_state_dict(live, strict=False)


class Trainer(object):
    """The reference Trainer's surface (src/DADiff.py:1506-1966): `train`, `save`, `load`, `sample`, `test`,
    `.accelerator.is_local_main_process`, `.results_folder`, `.train_logger`.  Unlike the reference (whose datasets glob
    private paths inside the class), the datasets are passed in: `dataset` (evaluation) is any object with
    `__len__`, `__getitem__ -> [ndct, ldct]` ((1,H,W) tensors in [0,1]) and `load_name(i)`; `train_dataset` needs the first two.
    `augment=True` applies the reference's RandomFlip + RandomRotate90 to every training pair (data/pdf_dataset.py:521-545), both
    images under one transform, drawn per item by diffusion_train.train_augment; `augment_flip` is ignored, as before.
    `crop_size` (an int or (h, w), multiples of 2 ** (levels - 1) of the U-Net; None: whole slices) trains on the reference's
    CropToFixed patches (data/transforms.py:196-249): every training pair is cut to the window diffusion_train.train_crop draws
    per item, reflect-padded where the slice is smaller, before the flip / rot90, which then needs a square crop for its odd
    rotations and no longer square slices; sample() and test() keep whole slices (test(tile=...) samples them as tiles of that size).
    `train_dataset` may be a data.DeviceSliceStore: train() then gathers (and augments) every micro-batch on the device and
    uploads no image.  `seed` keys what train() draws (diffusion_train.train_batch_indices / train_t_and_seeds / train_augment),
    `log_every` is how often the loss is read back from the device.
    `optimizer`: None or 'adam' is clip + Adam(`adam_betas`) on one U-Net, and train() / save() raise NotImplementedError for
    two; 'radam' is the reference's optimiser of two U-Nets (src/DADiff.py:1598-1602, 1707): one diffusion_train.ClipRAdamEMA
    with `radam_betas` (RAdam's defaults, as there) over the trainable parameters of every U-Net -- one clip over both, both
    updates and the one EMA in three launches -- and a checkpoint with 'opt0' and 'opt1' (diffusion_train.CHECKPOINT_KEYS_2).
    It is opt-in because the raising default is pinned by tests.  On one U-Net 'radam' is the reference's
    commented-out alternative (line 1594): the checkpoint keeps its five keys, 'opt0' in RAdam's layout.
    `val_dataset` (as train_dataset, or a data.DeviceSliceStore) is what validate() evaluates the EMA model on, forward-only: the
    held-out loss and the one-step PSNR / RMSE per noise band of `val_bands` (increasing edges inside [0, T]), on the first
    `val_items` items (None: all), keyed by `val_seed`, `val_batch_size` (item, band) pairs per launch sequence.  train() calls
    it every `validate_every` steps (0: never) and, with `keep_best`, saves model-best.pt whenever a validation beats every
    earlier one of this process.  All of it is off by default.  `val_crop_size` (an int or (h, w); None: whole slices) makes
    validate() evaluate the centred window of that size of every held-out slice -- the reference's CropToFixed(Center=True),
    origin (n - c) // 2 per axis -- which is how a model trained with `crop_size` was trained; a crop larger than the slice
    raises.
    `data_parallel=True` (off by default; `process_group` None: the default group) trains on the W ranks of an initialised
    torch.distributed group, one process per GPU, the reference's accelerate / DDP run (src/DADiff.py:1546-1623, 1705-1720).
    init_process_group is the caller's job (give it a finite timeout=, so that a lost peer ends in an error).  Micro-batch a of
    rank r is global micro-batch a W + r of A W, A = gradient_accumulate_every per rank: that number and that count key the
    indices, t, seeds, codes and windows, and the loss scale is 1 / (A W); diffusion_train.GradReducer adds the ranks' gradients
    in rank order, so that every parameter, EMA tensor, optimiser tensor and logged loss is bit for bit that of one process with
    gradient_accumulate_every = A W, whatever W.  Batch semantics: the reference's split_batches=True splits one batch of
    train_batch_size over the ranks; here a rank keeps train_batch_size and A W counts the micro-batches of a step.  Rank 0's
    model and buffers are broadcast once when training is set up; a DeviceSliceStore is held whole by every rank; previews,
    validate() and the checkpoint file are rank 0's, save() is called by every rank and ends in a barrier and check_replicas(),
    load(for_training=True) runs on every rank.  `split_batches` itself is ignored, as before.
    `ssim_weight` (None: the model's own attribute, 0.0 unless it was constructed otherwise; a finite number >= 0 sets it on the
    model and on the EMA copy) adds diffusion_train.structural_loss, 1 - SSIM of the one-step estimate under that weight, to the
    loss of the U-Net that predicts the residual or x0, inside that loss's autograd node: augment, crop_size (a crop below 6
    raises), optimizer='radam' and data_parallel see a loss and a gradient as before.  Like loss_type it is a setting of the
    constructor and no part of a checkpoint: a resumed run must be given it again.  `val_ssim=True` makes validate() report the
    one-step SSIM ("ssim", per U-Net and band) beside the PSNR and RMSE; best-checkpoint selection does not read it."""

    def __init__(self, opt, diffusion_model, folder=None, *, train_batch_size=16, gradient_accumulate_every=1,
                 augment_flip=True, train_lr=1e-4, train_num_steps=100000, ema_update_every=10, ema_decay=0.995,
                 adam_betas=(0.9, 0.99), save_and_sample_every=1000, num_samples=25, results_folder=".results/sample",
                 amp=False, fp16=False, split_batches=True, convert_image_to=None, condition=False, sub_dir=False,
                 equalizeHist=False, crop_patch=False, generation=False, num_unet=2, checkpoint_folder=None,
                 is_train=True, train_logger=None, dataset=None, device=None, train_dataset=None, seed=0, log_every=100,
                 augment=False, crop_size=None, optimizer=None, radam_betas=(0.9, 0.999), val_crop_size=None, data_parallel=False,
                 process_group=None, ssim_weight=None, val_ssim=False, val_dataset=None,
                 validate_every=0, val_bands=(0, 250, 500, 750, 1000), val_items=None, val_seed=0, val_batch_size=8, keep_best=False):
        import logging
        import os as _os
        self.data_parallel, self.process_group = bool(data_parallel), process_group
        self.world, self.rank = 1, 0
        if self.data_parallel:
            import torch.distributed as dist
            if not (dist.is_available() and dist.is_initialized()):
                raise RuntimeError("Trainer: data_parallel=True needs an initialised process group: call "
                                   "torch.distributed.init_process_group (with a finite timeout=) before the constructor")
            self.world, self.rank = dist.get_world_size(process_group), dist.get_rank(process_group)
        self._reducer = None                 # diffusion_train.GradReducer, made with the optimiser
        self.fingerprints = None             # with data_parallel: every rank's fingerprint at the last replica check
        if optimizer not in (None, "adam", "radam"):
            raise RuntimeError(f"Trainer: optimizer must be None, 'adam' or 'radam' (got {optimizer!r})")
        if len(tuple(radam_betas)) != 2 or not all(isinstance(b, (int, float)) and 0 <= b < 1 for b in radam_betas):
            raise RuntimeError(f"Trainer: radam_betas must be two numbers in [0, 1) (got {radam_betas!r})")
        self.optimizer, self.radam_betas = optimizer or "adam", tuple(float(b) for b in radam_betas)
        self.val_bands = dt.check_bands("Trainer", val_bands, getattr(diffusion_model, "num_timesteps", 1000))
        is_int = lambda v: isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))
        if not is_int(validate_every) or validate_every < 0 or not is_int(val_batch_size) or not 1 <= val_batch_size <= 65535 or \
                not is_int(val_seed) or not (val_items is None or (is_int(val_items) and val_items >= 1)):
            raise RuntimeError(f"Trainer: invalid validation arguments validate_every={validate_every!r} val_items={val_items!r} "
                               f"val_seed={val_seed!r} val_batch_size={val_batch_size!r} (integers; validate_every >= 0, val_items "
                               f"None or >= 1, 1 <= val_batch_size <= 65535)")
        if validate_every > 0 and val_dataset is None:
            raise RuntimeError(f"Trainer: validate_every={validate_every} needs a val_dataset")
        self.val_dataset, self.validate_every, self.val_items = val_dataset, int(validate_every), val_items
        self.val_seed, self.val_batch_size, self.keep_best = int(val_seed), int(val_batch_size), bool(keep_best)
        self.val_log = []                    # validate()'s results of this process, in order; not part of a checkpoint
        self.best = None                     # with keep_best: the entry of val_log that save("best") was last called for
        self._val_store = None               # val_dataset on the device, made at the first validate()
        self.val_crop_size = None if val_crop_size is None else dt.crop_pair("Trainer", val_crop_size, "val_crop_size")
        if self.val_crop_size is not None and min(self.val_crop_size) < 1:
            raise RuntimeError(f"Trainer: val_crop_size {self.val_crop_size} must be positive")
        self.crop_size = None
        if crop_size is not None:
            from .data import crop_pair
            ch, cw = crop_pair("Trainer", crop_size, "crop_size")
            unet = getattr(getattr(diffusion_model, "model", None), "unet0", None)
            step = 2 ** (len(getattr(unet, "dim_mults", (1,))) - 1)
            if ch < 1 or cw < 1 or ch % step or cw % step:
                raise RuntimeError(f"Trainer: crop_size {ch} x {cw} must be positive multiples of {step} (the U-Net has "
                                   f"{len(getattr(unet, 'dim_mults', (1,)))} levels)")
            self.crop_size = (ch, cw)
        self.opt = opt
        self.checkpoint_folder = checkpoint_folder or "."
        self.results_folder = self.checkpoint_folder + "/sample"
        _os.makedirs(self.results_folder, exist_ok=True)
        assert int(math.sqrt(num_samples)) ** 2 == num_samples, "number of samples must have an integer square root"
        self.num_samples = num_samples
        self.condition = condition
        self.num_unet = num_unet
        self.sub_dir, self.crop_patch = sub_dir, crop_patch
        self.image_size = diffusion_model.image_size
        self.device = torch.device(device or ("cuda" if torch.cuda.is_available() else "cpu"))
        self.accelerator = _Accel(self.device, process_group, self.data_parallel)
        self.model = diffusion_model.to(self.device)
        self.ema = _EMAView(self.model)      # inference uses the EMA weights (src/DADiff.py:1818-1822)
        self.ssim_weight, self.val_ssim = None, bool(val_ssim)
        if ssim_weight is not None:          # a constructor setting like loss_type: on the model (and on the EMA copy, made of it)
            self.ssim_weight = dt.check_ssim_weight("Trainer", ssim_weight)
            if self.ssim_weight > 0 and self.crop_size is not None and min(self.crop_size) < 6:
                raise RuntimeError(f"Trainer: ssim_weight={self.ssim_weight} with crop_size {self.crop_size[0]} x {self.crop_size[1]}: the "
                                   "structural term's 11-tap window (reflect padding of 5) needs crops of at least 6 x 6")
            self.model.ssim_weight = self.ssim_weight
        self.sample_dataset = dataset if dataset is not None else folder
        self.train_logger = train_logger or logging.getLogger("founddiff_amd")
        self.step = 0
        self.train_dataset = train_dataset
        self.batch_size, self.gradient_accumulate_every = int(train_batch_size), int(gradient_accumulate_every)
        self.train_lr, self.adam_betas, self.train_num_steps = train_lr, tuple(adam_betas), int(train_num_steps)
        self.ema_decay, self.ema_update_every = ema_decay, int(ema_update_every)
        self.save_and_sample_every = int(save_and_sample_every)
        self.seed, self.log_every = int(seed), int(log_every)
        self.augment = bool(augment)
        self.opt0 = None                     # ClipAdamEMA, made with the EMA copy at the first train() / save() / load(for_training=True)
        self.losses = None                   # the last step's losses, on the device
        self.loss_log = []                   # (step, [loss per U-Net]) of every logged step (the last 1024), as floats
        self.batch_log = []                  # a debugging aid: the dataset indices train() drew, one list per micro-batch (the
                                             # last 1024); diffusion_train.train_batch_indices gives the same without a run
        self._stale = False                  # a step has written the weights since the engines were packed
        self.condition_type = 2
        self.test_running_psnr, self.test_running_ssim, self.test_running_rmse = [], [], []

    def load(self, milestone, for_training=False):
        """Read `<ckpt>/sample/model-N.pt` = {'step','model','opt0','ema','scaler'}
        (src/DADiff.py:1648-1669).  The EMA weights win when present; a missing file is skipped
        silently like the reference does.  for_training=True resumes instead: the online model takes 'model', the EMA copy
        'ema', the optimiser 'opt0', and the step and EMA counters are restored, so that train() continues as the run that
        saved would have."""
        from pathlib import Path
        path = Path(self.results_folder + "/" + f"model-{milestone}.pt")
        if not path.exists():
            return
        data = torch.load(str(path), map_location="cpu", weights_only=False)
        if for_training:
            index, n = self._setup_training()
            if self._two_unets():
                step, model_sd, ema_sd, opt_sd = dt.checkpoint_unpack2(data, index, self._unet_index())
            else:
                step, model_sd, ema_sd, opt_sd = dt.checkpoint_unpack(data, index, n, optimizer=self.optimizer)
            load_weights(self.model, model_sd, f"{path}['model']")
            load_weights(self.ema.ema_model, ema_sd, f"{path}['ema']")
            self.model.to(self.device)
            self.ema.ema_model.to(self.device)
            self.opt0.load_state_dict(opt_sd)
            self.step = step
            self._stale = False
            self.model.weights_changed()
            self.ema.ema_model.weights_changed()
            print("load model - " + str(path))
            return
        load_weights(self.model, data["model"], f"{path}['model']")
        self.step = data.get("step", 0)
        ema = data.get("ema")
        if ema:
            live = {k[len("ema_model."):]: v for k, v in ema.items() if k.startswith("ema_model.")}
            if live:
                load_weights(self.model, live, f"{path}['ema']")
        self.model.to(self.device)
        getattr(self.model, "weights_changed", lambda: None)()
        if self.ema.ema_model is not self.model:
            # train() has made the EMA copy, and sample() / test() read it: it takes the same winning weights
            self.ema.ema_model.load_state_dict(self.model.state_dict())
            self.ema.ema_model.to(self.device)
            self.ema.ema_model.weights_changed()
            self._stale = False
        print("load model - " + str(path))

    # ---- training (src/DADiff.py:1626-1646, 1673-1763)
    def _setup_training(self):
        """The EMA copy and the optimiser, made once: (the places of the trainable parameters in diffusion.parameters(), their
        number).  Until here self.ema.ema_model is self.model."""
        dif = self.model
        if objectives.num_unet(dif.model) != 1 and self.optimizer != "radam":
            raise NotImplementedError("Trainer.train: two U-Nets are optimised with RAdam in the reference: pass optimizer='radam' "
                                      "(the default, Adam, trains one U-Net; DESIGN.md section 8)")
        dif.model.trainable()
        params = list(dif.parameters())
        index = [i for i, p in enumerate(params) if p.requires_grad]
        if self.opt0 is None:
            if self.device.type != "cuda":
                raise RuntimeError("Trainer.train: the model must live on the GPU (there is no CPU path)")
            if self.data_parallel:
                # once: every replica starts from rank 0's model and buffers; from here on identical gradients keep them identical
                from .parallel import broadcast_tensors
                broadcast_tensors(list(dif.parameters()) + list(dif.buffers()), 0, self.process_group)
                if self.ema.ema_model is not dif:
                    broadcast_tensors(list(self.ema.ema_model.parameters()) + list(self.ema.ema_model.buffers()), 0, self.process_group)
                dif.weights_changed()
            if self.ema.ema_model is dif:
                self.ema = _EMAView(dif.clone())
            if self.ssim_weight is not None:
                self.ema.ema_model.ssim_weight = self.ssim_weight
            eparams = list(self.ema.ema_model.parameters())
            cls, betas = (dt.ClipRAdamEMA, self.radam_betas) if self.optimizer == "radam" else (dt.ClipAdamEMA, self.adam_betas)
            self.opt0 = cls([params[i] for i in index], [eparams[i] for i in index], lr=self.train_lr, betas=betas, max_norm=1.0,
                            ema_beta=self.ema_decay, ema_update_every=self.ema_update_every)
            if self.data_parallel:
                self._reducer = dt.GradReducer(self.opt0, self.process_group)
        return index, len(params)

    def fingerprint(self):
        """an int64 sum of the parameters, the EMA copy's, the optimiser's moments and its step counts, each viewed as int32: equal
        on two replicas whose tensors are bitwise equal (and almost surely different otherwise).  Reads the device."""
        self._setup_training()
        tensors = [p.detach() for p in self.model.parameters()] + [p.detach() for p in self.ema.ema_model.parameters()] + \
            [self.opt0._m, self.opt0._v, self.opt0._steps]
        tot = torch.zeros((), dtype=torch.int64, device=self.device)
        for t in tensors:
            if t.element_size() == 4 and t.numel():
                tot = tot + t.contiguous().view(-1).view(torch.int32).sum(dtype=torch.int64)
        return int(tot.item()) + int(self.opt0.ema_step)

    def check_replicas(self):
        """data_parallel: every rank's fingerprint() gathered on every rank (self.fingerprints); RuntimeError on every rank if two
        differ -- the replicas have drifted apart, which identical gradients and identical optimisers cannot do."""
        if not self.data_parallel:
            return
        from .parallel import gather_int64
        self.fingerprints = gather_int64(self.fingerprint(), self.device, self.process_group)
        if len(set(self.fingerprints)) != 1:
            raise RuntimeError(f"Trainer: the replicas differ at step {self.step}: fingerprints per rank {self.fingerprints} "
                               f"(parameters, EMA and optimiser state as int32 sums)")

    def _two_unets(self):
        return objectives.num_unet(self.model.model) == 2

    def _unet_index(self):
        """the places of unet0.parameters() and of unet1.parameters() in diffusion.parameters(), each in its U-Net's order
        (diffusion_train.checkpoint_pack2)"""
        place = {id(p): i for i, p in enumerate(self.model.parameters())}
        return tuple([place[id(p)] for p in u.parameters()] for u in (self.model.model.unet0, self.model.model.unet1))

    def _fresh_engines(self):
        """before anything samples after a step has written the weights"""
        if self._stale:
            self.model.weights_changed()
            if self.ema.ema_model is not self.model:
                self.ema.ema_model.weights_changed()
            self._stale = False

    def train(self):
        """The reference's loop (src/DADiff.py:1683-1732) from self.step to train_num_steps: gradient_accumulate_every micro-batches
        through diffusion_train.train_step (clip 1.0, Adam, zero_grad, the EMA), a preview from the EMA model every
        save_and_sample_every steps and save() on the reference's schedule (its FID run is not built).  Micro-batch m of step s,
        its t, its noise and (with augment) its flip / rot90 codes are functions of (seed, s, m) alone; the losses stay on the
        device and are read every log_every steps.  From a data.DeviceSliceStore, or with augment or crop_size, a micro-batch is a
        diffusion_train.StoreBatch: its indices, codes, windows, t and seeds go up as one table and nothing waits for the host; a
        host dataset without augment and crop_size is loaded, stacked and uploaded as before.
        With validate_every > 0 every validate_every-th step is followed by validate(), which reads the weights and writes none:
        the run's tensors and counters are those of the same run without it.  With keep_best a validation that beats every
        earlier one of this process is followed by save("best") (_keep_best).  val_log and best are not part of a checkpoint,
        whose keys stay diffusion_train.CHECKPOINT_KEYS (CHECKPOINT_KEYS_2 for two U-Nets): a resumed run starts with both empty
        and re-establishes its best at its first validation, overwriting model-best.pt whatever the interrupted run had reached.
        optimizer='radam' runs the same loop around ClipRAdamEMA, on one U-Net or two; the log line then has loss_unet1 too.
        With data_parallel every rank runs this loop over its own micro-batch numbers (a W + rank) and the gradients meet in
        diffusion_train.GradReducer; rank 0 logs, previews and validates, every rank joins save() and the replica check that
        also ends the run.  loss_log keeps (step, losses) of every logged step on every rank."""
        from .data import DeviceSliceStore
        self._setup_training()
        ds = self.train_dataset
        if ds is None or len(ds) < 1:
            raise RuntimeError("Trainer.train: give the constructor a train_dataset (__len__, __getitem__ -> [ndct, ldct])")
        if self.sample_dataset is None:
            self.sample_dataset = ds
        every, T = self.save_and_sample_every, self.model.num_timesteps
        # data_parallel: micro-batch a of this rank is global micro-batch a W + rank of the step's A W
        W, rank, main = self.world, self.rank, self.rank == 0
        acc = self.gradient_accumulate_every * W
        while self.step < self.train_num_steps:
            batches, ts, seeds = [], [], []
            for m in (dt.dp_micro(a, W, rank) for a in range(self.gradient_accumulate_every)):
                idx = dt.train_batch_indices(self.seed, self.step, m, self.batch_size, len(ds), acc)
                self.batch_log.append(idx)
                t, sd = dt.train_t_and_seeds(self.seed, self.step, m, idx, T)
                if isinstance(ds, DeviceSliceStore) or self.augment or self.crop_size:
                    store, local = (ds, idx) if isinstance(ds, DeviceSliceStore) else \
                        (DeviceSliceStore.from_items([ds[i] for i in idx], self.device), list(range(len(idx))))
                    crop = self.crop_size
                    square = store.H == store.W if crop is None else crop[0] == crop[1]
                    codes = dt.train_augment(self.seed, self.step, m, idx, square) if self.augment else None
                    windows = dt.train_crop(self.seed, self.step, m, idx, store.H, store.W, crop) if crop else None
                    batches.append(dt.StoreBatch(store, local, codes, windows, crop))
                    ts.append(t)
                    seeds.append(sd)
                    continue
                items = [ds[i] for i in idx]
                batches.append([torch.stack([it[j] for it in items]).float().to(self.device) for j in range(2)])
                ts.append(torch.from_numpy(t).to(self.device))
                seeds.append(torch.from_numpy(sd).to(self.device))
            del self.batch_log[:-1024]
            self.losses = dt.train_step(self.model, self.opt0, batches, t=ts, slice_seeds=seeds, step=self.step, reducer=self._reducer)
            self._stale = True
            self.step += 1
            if self.log_every > 0 and self.step % self.log_every == 0:                 # the one synchronisation of these steps
                vals = [float(v) for v in self.losses]
                self.loss_log.append((self.step, vals))
                del self.loss_log[:-1024]
                if main:
                    self.train_logger.info("Iters: [%d/%d], " % (self.step, self.train_num_steps) +
                                           ", ".join("loss_unet%d: %.6f" % (u, v) for u, v in enumerate(vals)))
            if self.validate_every > 0 and self.step % self.validate_every == 0:
                res = self.validate() if main else None
                if self.keep_best and not self.data_parallel:
                    self._keep_best(res)
                elif self.keep_best:                                                   # rank 0 decides, every rank joins save()
                    from .parallel import gather_int64
                    if gather_int64(int(self._is_best(res)) if main else 0, self.device, self.process_group)[0]:
                        self.save("best")
            if self.step % every == 0:
                milestone = self.step // every
                if main:
                    self.sample(milestone)
                if self.step > every * 10 * 4 and self.step % (every * 10) == 0:
                    self.save(milestone)
        self.check_replicas()
        print("training complete")

    def save(self, milestone):
        """`<results>/model-N.pt` = {'step', 'model', 'opt0', 'ema', 'scaler': None} (src/DADiff.py:1626-1646;
        diffusion_train.checkpoint_pack)."""
        index, n = self._setup_training()
        if self.data_parallel:
            # every rank calls save(): rank 0 writes the file (its keys and layout are the single process's: a checkpoint written
            # at W ranks of A micro-batches resumes at any W', A' with A' W' = A W), then a barrier and the replica check
            if self.rank == 0:
                self._write_checkpoint(milestone, index, n)
            self.accelerator.wait_for_everyone()
            self.check_replicas()
            return
        self._write_checkpoint(milestone, index, n)

    def _write_checkpoint(self, milestone, index, n):
        ema_sd = {k: v.detach().clone() for k, v in self.ema.ema_model.state_dict().items()}
        model_sd = {k: v.detach().clone() for k, v in self.model.state_dict().items()}
        if self._two_unets():
            data = dt.checkpoint_pack2(self.step, model_sd, ema_sd, self.opt0.state_dict(), index, self._unet_index())
        else:
            data = dt.checkpoint_pack(self.step, model_sd, ema_sd, self.opt0.state_dict(), index, n)
        torch.save(data, self.results_folder + "/" + f"model-{milestone}.pt")

    # ---- held-out evaluation during a run (the reference has none before its full test() at step 50 000, src/DADiff.py:1731-1745)
    @torch.no_grad()
    def validate(self, precision="fp32"):
        """The EMA model (the model itself until train() copies it) on val_dataset: whole slices (with val_crop_size their centred
        window of that size, through the store's explicit windows), no augmentation, the first val_items of them (None: all).
        Every item is evaluated once per noise band of val_bands, at the t and with the
        noise diffusion_train.val_draws keys by (val_seed, item, band), in batches of val_batch_size (item, band) pairs through
        diffusion_train.StoreBatch and ResidualDiffusion.eval_items on the `precision` engine; a host dataset goes to the device
        once, at the first call.  With val_ssim the dict has "ssim" too, shaped as psnr: the SSIM of the same one-step estimate by
        the definition test() reports.  Returns {"step", "bands", "loss", "psnr", "rmse", "n"}: loss, psnr and rmse are lists per
        U-Net, then per band, of diffusion_train.val_summary's means (psnr and rmse of the one-step denoising error, NaN for an
        output that is no residual), n the items per band; the dict is appended to val_log and logged, one line per band and
        one over all bands.  Deterministic: the numbers depend on the weights alone, not on the step, the training seed or
        val_batch_size."""
        from .data import DeviceSliceStore
        fn = "Trainer.validate"
        if self.val_dataset is None:
            raise RuntimeError(f"{fn}: give the constructor a val_dataset (__len__, __getitem__ -> [ndct, ldct])")
        if self.device.type != "cuda":
            raise RuntimeError(f"{fn}: the model must live on the GPU (there is no CPU path)")
        if self._val_store is None:
            ds = self.val_dataset
            self._val_store = ds if isinstance(ds, DeviceSliceStore) else DeviceSliceStore.from_dataset(ds, self.device)
        store, ema = self._val_store, self.ema.ema_model
        crop = self.val_crop_size
        if crop is not None and (crop[0] > store.H or crop[1] > store.W):
            raise RuntimeError(f"{fn}: val_crop_size {crop[0]} x {crop[1]} is larger than the slices {store.H} x {store.W}")
        n = len(store) if self.val_items is None else min(int(self.val_items), len(store))
        item, band, t, seeds = dt.val_draws(self.val_seed, range(n), self.val_bands, ema.num_timesteps)
        self._fresh_engines()
        rows = []
        for s in range(0, len(item), self.val_batch_size):
            sl = slice(s, s + self.val_batch_size)
            if crop is None:
                batch = dt.StoreBatch(store, item[sl])
            else:                                             # the centred window: CropToFixed(Center=True), origin (n - c) // 2
                win = np.tile(np.array([[(store.H - crop[0]) // 2, (store.W - crop[1]) // 2]], dtype=np.int64), (len(item[sl]), 1))
                batch = dt.StoreBatch(store, item[sl], None, win, crop)
            kw = {"ssim": True} if self.val_ssim else {}              # off: the call a model without the keyword has always got
            rows.append(ema.eval_items(batch, t[sl], slice_seeds=seeds[sl], precision=precision, **kw))
        nb = len(self.val_bands) - 1
        per_unet = [torch.cat([r[u] for r in rows]).cpu().numpy() for u in range(len(rows[0]))]      # the one synchronisation
        sums = [dt.val_summary(v, band, nb) for v in per_unet]
        res = {"step": self.step, "bands": list(self.val_bands), "loss": [s["loss"] for s in sums], "psnr": [s["psnr"] for s in sums],
               "rmse": [s["rmse"] for s in sums], "n": sums[0]["n"]}
        if self.val_ssim:
            res["ssim"] = [s["ssim"] for s in sums]
        self.val_log.append(res)
        info = self.train_logger.info
        for u, s in enumerate(sums):
            for k in range(nb):
                extra = ", val_ssim: %.6f" % s["ssim"][k] if self.val_ssim else ""
                info("Iters: [%d/%d], unet%d t in [%d, %d): val_loss: %.6f, val_psnr: %.4f, val_rmse: %.6f%s (%d items)" % (
                    self.step, self.train_num_steps, u, self.val_bands[k], self.val_bands[k + 1], s["loss"][k], s["psnr"][k],
                    s["rmse"][k], extra, s["n"][k]))
            tot = dt.val_summary(per_unet[u], np.zeros(len(band), dtype=np.int64), 1)
            info("Iters: [%d/%d], unet%d val_loss: %.6f, val_psnr: %.4f, val_rmse: %.6f%s" % (
                self.step, self.train_num_steps, u, tot["loss"][0], tot["psnr"][0], tot["rmse"][0],
                ", val_ssim: %.6f" % tot["ssim"][0] if self.val_ssim else ""))
        return res

    @staticmethod
    def _val_score(res):
        """("psnr", the mean one-step PSNR over the items of every band) where a U-Net has a residual output, else ("loss", the
        mean loss over items, bands and U-Nets)"""
        mean = lambda per_band: float(np.average(per_band, weights=res["n"]))
        psnr = [mean(p) for p in res["psnr"] if not np.isnan(p).all()]
        if psnr:
            return "psnr", float(np.mean(psnr))
        return "loss", float(np.mean([mean(v) for v in res["loss"]]))

    def _keep_best(self, res):
        """save("best") if `res` (a result of validate()) beats every earlier one of this process: a higher mean one-step PSNR,
        or a lower mean loss where no U-Net has a residual output.  self.best = {"step", "metric", "value"} of the winner."""
        if self._is_best(res):
            self.save("best")
            self.train_logger.info("Iters: [%d/%d], best val_%s so far: %.6f, saved model-best.pt" % (
                self.step, self.train_num_steps, self.best["metric"], self.best["value"]))

    def _is_best(self, res):
        """whether `res` beats every earlier validation of this process; self.best then becomes its entry"""
        metric, value = self._val_score(res)
        old = self.best
        if old is None or np.isnan(old["value"]) or (value > old["value"] if metric == "psnr" else value < old["value"]):
            self.best = {"step": res["step"], "metric": metric, "value": value}
            return True
        return False

    # anatomy groups of the reference's 2020 test list, in item order: (name, slices per dose level); each holds
    # 4 dose levels back to back (src/DADiff.py:1918-1950).  "head" is taken from the END of the list, as there.
    test_groups = (("ab", 290), ("lung", 637), ("head", 159))

    @torch.no_grad()
    def sample(self, milestone, last=True, FID=False):
        """Preview grid of [NDCT, LDCT, x_T, output] in the HU display window, `<results>/sample-N.png`
        (src/DADiff.py:1765-1815); with FID, one PNG per generated image, `milestone` advancing."""
        from .data import hu_window, save_image
        n = min(self.num_samples, len(self.sample_dataset))
        items = [self.sample_dataset[i] for i in range(n)]
        show = [torch.stack([it[j] for it in items]).to(self.device) for j in range(len(items[0]))]
        self._fresh_engines()
        outs = list(self.ema.ema_model.sample(show[1:], batch_size=n, last=last))      # (the model itself until train() copies it)
        all_images_list = show + outs
        all_images = hu_window(torch.cat(all_images_list, dim=0))
        nrow = int(math.sqrt(self.num_samples)) if last else all_images.shape[0]
        if FID:
            for i in range(n):
                file_name = f"sample-{milestone}.png"
                save_image(all_images_list[0][i].unsqueeze(0), os.path.join(self.results_folder, file_name), nrow=1)
                milestone += 1
                if milestone >= getattr(self, "total_n_samples", 50000):
                    break
        else:
            file_name = f"sample-{milestone}.png"
            save_image(all_images, self.results_folder + "/" + file_name, nrow=nrow)
        print("sampe-save " + file_name)
        return milestone

    @staticmethod
    def image_file_name(file_name):
        """PNG name of a result (src/DADiff.py:1904-1907): quarter-dose files keep the part before the first
        dot, simulated-dose files (`...-0.25-0012.npy`) keep the dose fraction's dot."""
        if "quarter" in file_name:
            return file_name.split(".")[0] + ".png"
        return file_name.split(".")[0] + "." + file_name.split(".")[1] + ".png"

    def _log_groups(self):
        """Per-anatomy and per-dose means of the running metrics (src/DADiff.py:1918-1950), same slicing rule
        and log lines; groups the evaluated list does not reach log nan, as np.mean of an empty slice does."""
        def mean(v):
            return float(np.mean(v)) if len(v) else float("nan")
        P, S, R = self.test_running_psnr, self.test_running_ssim, self.test_running_rmse
        out, off = {}, 0
        for gi, (name, length) in enumerate(self.test_groups):
            if gi == len(self.test_groups) - 1:
                sl = slice(-length * 4, None)
            else:
                sl = slice(off, off + length * 4)
            gp, gs, gr = P[sl], S[sl], R[sl]
            self.train_logger.info("(%s average mean: psnr: %.4f, ssim: %.4f,rmse: %.4f)" % (name, mean(gp), mean(gs), mean(gr)))
            out[name] = {"mean": (mean(gp), mean(gs), mean(gr)), "dose": []}
            for i in range(4):
                d = slice(int(i * length), int((i + 1) * length))
                row = (mean(gp[d]), mean(gs[d]), mean(gr[d]))
                out[name]["dose"].append(row)
                self.train_logger.info("(%s\u2014\u2014\u2014\u2014dose: %2d,average: psnr: %.4f, ssim: %.4f,rmse: %.4f)" % ((name, i) + row))
            off += length * 4
        return out

    @torch.no_grad()
    def test(self, sample=False, last=True, FID=False, batch_size=1, n_samples=1, ensemble_seed=0, tile=None, overlap=0,
             tile_condition="tile", tile_fuse="final", tiled_ensemble=False, *, quantiles=None, estimate="mean", orientations=None,
             interval_scale=None):
        """Evaluation loop of src/DADiff.py:1817-1966: init() the schedule, denoise every slice,
        PSNR/SSIM/RMSE vs NDCT (on device), np.save each output in [0,1], per-anatomy / per-dose means.
        `batch_size` > 1 batches independent slices (the reference uses 1).  `sample=True` keeps the
        reference's branch that returns inputs + outputs without metrics; without `condition` the loop is the
        reference's unconditional `self.sample` rounds (100, or up to 50000 images with FID).
        `n_samples` > 1: every slice is denoised as an ensemble (ResidualDiffusion.sample_ensemble) under the slice seed
        `ensemble_seed` + its dataset index; the metrics and the saved image are those of the ensemble mean, and outside
        training the per-pixel standard deviation is saved beside it as `<name>_std.npy`.
        `tile` (an int or (th, tw); None: whole slices, as ever): every slice is sampled as overlapping tiles
        (ResidualDiffusion.sample_tiled with `overlap`, condition=`tile_condition` and fuse=`tile_fuse`) under the slice seed
        `ensemble_seed` + its dataset index; the metrics and the saved image are those of the blended slice.  Ensembles of tiled samples
        (n_samples > 1 with a tile) are opt-in: `tiled_ensemble=True` runs sample_ensemble(tile=...) under the same slice seeds and
        scores and saves the ensemble mean and `<name>_std.npy` as above; without the switch the combination raises (the raising
        default is pinned by tests).  last=False with a tile is not built and raises.
        `quantiles` (keyword-only, with n_samples > 1): a sequence of levels in [0, 1]; outside training every level's map of
        the ensemble (sample_ensemble(quantiles=...)) is saved beside the image as `<name>_qNNNN.npy`, NNNN the level in
        per-mille (0.05: `_q0050`; levels that collide there raise), cropped like `_std`.  With at least two levels the share of
        each slice's NDCT pixels inside [lowest level, highest level] (metrics.interval_coverage) goes to
        `self.test_running_coverage`, and its mean is logged next to the nominal highest - lowest.
        `estimate` (keyword-only): "mean", or "median" (n_samples > 1): the metrics and the saved image are those of the ensemble's
        0.5 level, which joins the levels if it is not among them.
        `orientations` (keyword-only; None: all of the above): "d4", "flips" or a sequence of flip / rot90 codes; every slice is
        denoised as an orientation ensemble (sample_ensemble(orientations=...)) of n_samples >= 1 replicas under the same slice
        seeds, and scored and saved as an ensemble is; with n_samples=1 it is one sample of the oriented slice, turned back.  Not
        built together with a tile: it raises.
        `interval_scale` (keyword-only; None: all of the above, every launch, file, list and log line as it is): a number >= 0, or
        "calibrated" for the scale of `self.interval_calibration` (calibrate_intervals / load_interval_calibration), which raises
        if there is none or if its `settings` differ from this call's, naming the field.  It needs `quantiles` with at least two
        levels.  Per batch the interval [lowest level, highest level] is scaled around the estimate (metrics.interval_scale) and
        the NDCT pixels it covers are counted by the calibration's own criterion, score <= scale (bin 0 of
        metrics.interval_hist on the one-value grid [scale]): their share per slice goes to
        `self.test_running_coverage_calibrated`, the mean width per slice to `self.test_running_interval_width`, and outside
        training `<name>_lo.npy` and `<name>_hi.npy` are saved beside `<name>_std.npy`, cropped the same way.  One more log line
        gives the mean calibrated coverage, 1 - alpha when known, the mean width and that of the unscaled interval.  The `_qNNNN`
        maps and `test_running_coverage` stay those of the raw levels.  The guarantee of a calibration holds for slices exchangeable
        with its calibration slices: test on other patients than those calibrated on, with the same model and sampling settings."""
        qplan = _ensemble_plan("Trainer.test", n_samples, quantiles, estimate, tile, tiled_ensemble, orientations)
        if tile is not None and not last:
            raise RuntimeError("Trainer.test: tile with last=False is not built (sample_tiled returns the final image)")
        iplan = None
        if interval_scale is not None:
            if qplan is None or len(qplan.user) < 2:
                raise RuntimeError("Trainer.test: interval_scale needs quantiles with at least two levels (the interval that is scaled)")
            settings = _interval_settings(getattr(getattr(self, "ema", None), "ema_model", None), n_samples, qplan.user, estimate,
                                          None, tile, overlap, tile_condition, tile_fuse, orientations)
            if isinstance(interval_scale, str):
                if interval_scale != "calibrated":
                    raise RuntimeError(f"Trainer.test: interval_scale must be None, a number or 'calibrated' (got {interval_scale!r})")
                cal = getattr(self, "interval_calibration", None)
                if cal is None:
                    raise RuntimeError("Trainer.test: interval_scale='calibrated' needs a calibration: call calibrate_intervals or "
                                       "load_interval_calibration first")
                settings["floor"] = (cal.settings or {}).get("floor")
                for key, value in settings.items():
                    if (cal.settings or {}).get(key) != value:
                        raise RuntimeError(f"Trainer.test: the calibration is not valid for this call: {key} was "
                                           f"{(cal.settings or {}).get(key)!r} when it was made and is {value!r} now")
                iplan = _IntervalPlan(cal.scale, float(settings["floor"]), 1 - cal.alpha)
            else:
                if isinstance(interval_scale, bool) or not isinstance(interval_scale, (int, float, np.integer, np.floating)) or \
                        not 0 <= float(interval_scale) < float("inf"):
                    raise RuntimeError(f"Trainer.test: interval_scale must be None, a number >= 0 or 'calibrated' (got {interval_scale!r})")
                iplan = _IntervalPlan(float(interval_scale), INTERVAL_FLOOR, None)
        # batch_size 1 is the reference's loop: one slice per sample() call -> the kernel set for a lone slice (DAEngine
        # low_latency: same arithmetic, chunked scans at every level; outputs differ from a batched run by fp32
        # summation order).  The switch is only ever turned ON here (FOUNDDIFF_LOW_LATENCY=1 stays in force for any batch
        # size) and is restored on the way out, so later sample() calls on the same model are not affected.  Cost: the
        # low-latency engine is a second DAEngine (its own weight copy, workspaces and graphs) next to the default one.
        self._fresh_engines()
        unets = [u for u in objectives.unets_of(getattr(self.ema.ema_model, "model", None)) if hasattr(u, "low_latency")]
        saved = [u.low_latency for u in unets]
        try:
            if batch_size == 1 and int(n_samples) == 1 and tile is None and orientations is None:   # (an ensemble is a batch of replicas, a tiled slice
                for u in unets:                                           # a batch of tiles: the default kernel set)
                    u.low_latency = True
            tiled = None if tile is None else dict(tile=tile, overlap=overlap, tile_condition=tile_condition, tile_fuse=tile_fuse)
            return self._test(sample, last, FID, batch_size, int(n_samples), int(ensemble_seed), tiled, qplan, orientations, iplan)
        finally:
            for u, v in zip(unets, saved):
                u.low_latency = v

    def _test(self, sample, last, FID, batch_size, n_samples=1, ensemble_seed=0, tiled=None, qplan=None, orientations=None,
              iplan=None):
        """`tiled`: None, or the keyword arguments of sample_ensemble that make it tiled; `qplan`: None, or test()'s _QuantilePlan;
        `orientations`: None, or sample_ensemble's, which makes every slice an ensemble at any n_samples; `iplan`: None, or
        test()'s _IntervalPlan (then qplan has at least two of the caller's levels)"""
        from .metrics import compute_metrics
        model = self.ema.ema_model                   # inference uses the EMA weights (src/DADiff.py:1818-1822)
        model.init()
        print("test start")
        if not self.condition:
            if FID:
                import glob
                self.total_n_samples = 50000
                img_id = len(glob.glob(f"{self.results_folder}/*"))
                n_rounds = (self.total_n_samples - img_id) // self.num_samples + 1
            else:
                n_rounds = 100
            for i in range(n_rounds):
                if FID:
                    i = img_id
                img_id = self.sample(i, last=last, FID=FID)
            print("test end")
            return None
        self.test_running_psnr, self.test_running_ssim, self.test_running_rmse = [], [], []
        self.test_image_names = []
        q_names, q_cover = [], None
        if qplan is not None:
            self.test_running_coverage = []
            q_names = quantile_suffix(qplan.user)
            if len(qplan.user) >= 2:                           # the interval [lowest level, highest level] of the caller's levels
                q_cover = (qplan.user.index(min(qplan.user)), qplan.user.index(max(qplan.user)))
        if iplan is not None:
            self.test_running_coverage_calibrated, self.test_running_interval_width = [], []
            raw_width = []
        ens_kw = dict(tiled or {}, **({} if qplan is None else {"quantiles": qplan.levels}))
        if orientations is not None:
            ens_kw["orientations"] = orientations
        ds = self.sample_dataset
        for s in range(0, len(ds), batch_size):
            idx = list(range(s, min(s + batch_size, len(ds))))
            items = [ds[i] for i in idx]
            y = torch.stack([it[0] for it in items]).to(self.device)
            xs = [torch.stack([it[k] for it in items]).to(self.device) for k in range(1, len(items[0]))]
            y_std = y_q = cover = scaled = None
            if n_samples > 1 or orientations is not None:
                ens = model.sample_ensemble(xs, n_samples, slice_seeds=[ensemble_seed + i for i in idx], **ens_kw)
                y_pred, y_std = ens.mean, ens.std
                if qplan is not None:
                    y_q = ens.quantiles
                    if qplan.estimate is not None:             # estimate="median": the 0.5 level is scored and saved
                        y_pred = y_q[:, qplan.estimate]
                    if q_cover is not None and not sample:
                        cover = interval_coverage(y_q[:, q_cover[0]], y_q[:, q_cover[1]], y)[1]
                    if iplan is not None and not sample:
                        # the scaled interval around the estimate, and the pixels it holds by the calibration's own criterion:
                        # bin 0 of the one-value grid [scale] is score <= scale
                        maps = (y_pred, y_q[:, q_cover[0]], y_q[:, q_cover[1]])
                        lo_s, hi_s, width = interval_scale(*maps, iplan.scale, iplan.floor)
                        inside = interval_hist(*maps, y, [iplan.scale], iplan.floor)[:, 0].cpu().numpy()
                        scaled = (lo_s, hi_s, inside.astype("float64") / y[0].numel(), width.cpu().numpy(),
                                  interval_scale(*maps, 1.0, iplan.floor)[2].cpu().numpy())
            elif tiled is not None:
                outs = model.sample_tiled(xs, tiled["tile"], tiled["overlap"], slice_seeds=[ensemble_seed + i for i in idx],
                                          condition=tiled["tile_condition"], fuse=tiled["tile_fuse"])
                all_images_list = [y] + xs + list(outs)
                y_pred = outs[-1]
            elif sample:
                all_images_list = [y] + xs + list(model.sample(xs, batch_size=len(idx)))
                y_pred = all_images_list[-1]
            else:
                y_pred = list(model.sample(xs, batch_size=len(idx), last=last))[-1]
            if not sample:
                # src/DADiff.py:1872-1886: the metrics use the UNCROPPED prediction; crop_patch only crops what is saved
                m = compute_metrics(y_pred, y).cpu().numpy()
            y_save = y_pred
            if self.crop_patch and not sample:
                # the reference calls get_pad_size with its 1-based item counter (1826-1838, 1875): the last item would
                # index one past the end of a 0-based table, so the index is clamped
                pad = [tuple(ds.get_pad_size(min(i + 1, len(ds) - 1))) for i in idx]
                if len(set(pad)) != 1:
                    raise ValueError("crop_patch needs one pad size per batch (use batch_size=1)")
                h, w = y_pred.shape[-2:]
                y_save = y_pred[:, :, 0:h - pad[0][0], 0:w - pad[0][1]]
            for j, i in enumerate(idx):
                file_name = ds.load_name(i, sub_dir=self.sub_dir)
                self.test_image_names.append(self.image_file_name(file_name))
                if not sample:
                    self.test_running_psnr.append(m[j, 0])
                    self.test_running_ssim.append(m[j, 1])
                    self.test_running_rmse.append(m[j, 2])
                    print("(psnr: %.4f, ssim: %.4f,rmse:.%.4f) " % (m[j, 0], m[j, 1], m[j, 2]))
                    if cover is not None:
                        self.test_running_coverage.append(float(cover[j]))
                    if scaled is not None:
                        self.test_running_coverage_calibrated.append(float(scaled[2][j]))
                        self.test_running_interval_width.append(float(scaled[3][j]))
                        raw_width.append(float(scaled[4][j]))
                if not getattr(self.opt, "is_train", False) and not sample:
                    h, w = y_save.shape[-2:]
                    np.save(self.results_folder + "/" + file_name[:-4], y_save[j].detach().cpu().numpy().reshape(h, w))
                    if y_std is not None:                      # the spread of the ensemble, cropped like the image
                        np.save(self.results_folder + "/" + file_name[:-4] + "_std",
                                y_std[j, :, :h, :w].detach().cpu().numpy().reshape(h, w))
                    for qi, suffix in enumerate(q_names):      # the caller's levels, cropped like the image
                        np.save(self.results_folder + "/" + file_name[:-4] + suffix,
                                y_q[j, qi, :, :h, :w].detach().cpu().numpy().reshape(h, w))
                    if scaled is not None:                     # the scaled interval, cropped like the image
                        for suffix, t in (("_lo", scaled[0]), ("_hi", scaled[1])):
                            np.save(self.results_folder + "/" + file_name[:-4] + suffix,
                                    t[j, :, :h, :w].detach().cpu().numpy().reshape(h, w))
                    print("test-save " + file_name)
        if sample:
            print("test end")
            return None
        self.test_group_means = self._log_groups()
        self.train_logger.info("test_psnr: {:.4f}, test_ssim: {:.4f},test_rmse:{:.4f}".format(
            np.mean(self.test_running_psnr), np.mean(self.test_running_ssim), np.mean(self.test_running_rmse)))
        if q_cover is not None:
            self.train_logger.info("test_coverage: {:.4f} of the NDCT pixels inside [q{:g}, q{:g}] (nominal {:.4f})".format(
                np.mean(self.test_running_coverage), qplan.user[q_cover[0]], qplan.user[q_cover[1]],
                qplan.user[q_cover[1]] - qplan.user[q_cover[0]]))
        if iplan is not None:
            self.train_logger.info("test_coverage_calibrated: {:.4f} of the NDCT pixels inside the interval scaled by {:g} ({}), "
                                   "mean width {:.6f} (unscaled: {:.6f})".format(
                                       np.mean(self.test_running_coverage_calibrated), iplan.scale,
                                       "no calibration" if iplan.nominal is None else "calibrated for {:.4f}".format(iplan.nominal),
                                       np.mean(self.test_running_interval_width), np.mean(raw_width)))
        print("test end")
        return float(np.mean(self.test_running_psnr)), float(np.mean(self.test_running_ssim)), \
            float(np.mean(self.test_running_rmse))

    INTERVAL_CALIBRATION_FILE = "interval_calibration.json"

    @torch.no_grad()
    def calibrate_intervals(self, dataset=None, *, n_samples, quantiles, estimate="mean", alpha=0.1, bound="crc", delta=None,
                            grid=None, floor=INTERVAL_FLOOR, ensemble_seed=0, batch_size=1, items=None, tile=None, overlap=0,
                            tile_condition="tile", tile_fuse="final", tiled_ensemble=False, orientations=None):
        """One scale for the ensemble interval of this model, chosen on held-out slices so that the share of NDCT pixels the scaled
        interval misses is controlled (ensemble.risk_control: `alpha`, `bound` "crc" or "hoeffding" with `delta`).
        `dataset` (None: `val_dataset`) is read as test() reads its own: item -> [ndct, ldct].  The EMA model samples every one of
        the first `items` slices (None: all) as test(n_samples=, quantiles=, estimate=, tile..., orientations=) would, under the
        slice seeds `ensemble_seed` + index; l and u are the lowest and the highest of the caller's levels, the centre is the
        ensemble mean, or the 0.5 level under estimate="median".  Per batch metrics.interval_hist bins every pixel's score over
        `grid` (None: ensemble.interval_grid()) with the half-width floor `floor`; the counts stay on the device and are read back
        once.  Returns the IntervalCalibration, keeps it as `self.interval_calibration` (and the counts per slice, (N, G + 1), as
        `self.interval_counts`) and, on rank 0 outside training, writes `<results_folder>/interval_calibration.json`.  Its
        `settings` record what the scale is valid for: test(interval_scale="calibrated") refuses any other.  The guarantee is
        for slices exchangeable with those calibrated on: adjacent slices of one patient are not independent, so calibrate on
        patients other than those tested, and again for another model, sampler, step count or ensemble."""
        fn = "Trainer.calibrate_intervals"
        if quantiles is None or len(tuple(quantiles)) < 2:
            raise RuntimeError(f"{fn}: quantiles must hold at least two levels, the interval that is scaled (got {quantiles!r})")
        qplan = _ensemble_plan(fn, n_samples, quantiles, estimate, tile, tiled_ensemble, orientations)
        grid = check_interval_grid(interval_grid() if grid is None else grid)
        if not 0 < float(floor) < float("inf"):
            raise RuntimeError(f"{fn}: floor must be positive and finite (got {floor})")
        if not 0 < float(alpha) < 1 or bound not in ("crc", "hoeffding") or (bound == "hoeffding") != (delta is not None) or \
                (delta is not None and not 0 < float(delta) < 1):
            raise RuntimeError(f"{fn}: need 0 < alpha < 1 and bound 'crc', or 'hoeffding' with 0 < delta < 1 (got alpha={alpha!r} "
                               f"bound={bound!r} delta={delta!r})")
        is_int = lambda v: isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))
        if not is_int(batch_size) or batch_size < 1 or not (items is None or (is_int(items) and items >= 1)):
            raise RuntimeError(f"{fn}: batch_size must be an integer >= 1 and items None or an integer >= 1 (got {batch_size!r}, "
                               f"{items!r})")
        ds = dataset if dataset is not None else getattr(self, "val_dataset", None)
        if ds is None:
            raise RuntimeError(f"{fn}: no dataset: pass one, or construct the Trainer with val_dataset=")
        N = len(ds) if items is None else min(int(items), len(ds))
        if N < 1:
            raise RuntimeError(f"{fn}: the dataset is empty")
        self._fresh_engines()
        model = self.ema.ema_model
        model.init()
        settings = _interval_settings(model, n_samples, qplan.user, estimate, floor, tile, overlap, tile_condition, tile_fuse,
                                      orientations)
        lo_i, hi_i = qplan.user.index(min(qplan.user)), qplan.user.index(max(qplan.user))
        ens_kw = dict(quantiles=qplan.levels)
        if tile is not None:
            ens_kw.update(tile=tile, overlap=overlap, tile_condition=tile_condition, tile_fuse=tile_fuse)
        if orientations is not None:
            ens_kw["orientations"] = orientations
        counts, n_pixels = [], None
        for s in range(0, N, batch_size):
            idx = list(range(s, min(s + batch_size, N)))
            its = [ds[i] for i in idx]
            y = torch.stack([it[0] for it in its]).to(self.device)
            xs = [torch.stack([it[k] for it in its]).to(self.device) for k in range(1, len(its[0]))]
            ens = model.sample_ensemble(xs, int(n_samples), slice_seeds=[int(ensemble_seed) + i for i in idx], **ens_kw)
            centre = ens.mean if qplan.estimate is None else ens.quantiles[:, qplan.estimate]
            counts.append(interval_hist(centre, ens.quantiles[:, lo_i], ens.quantiles[:, hi_i], y, grid, floor))
            n_pixels = y[0].numel()
        self.interval_counts = torch.cat(counts).cpu().numpy()                     # the one read-back
        cal = risk_control(self.interval_counts, n_pixels, grid, alpha, bound, delta)._replace(settings=settings)
        self.interval_calibration = cal
        if self.accelerator.is_main_process and not getattr(self.opt, "is_train", False):
            import json
            with open(os.path.join(self.results_folder, self.INTERVAL_CALIBRATION_FILE), "w") as f:
                json.dump(cal._asdict(), f, indent=1)
                f.write("\n")
        self.train_logger.info("interval_calibration: scale {:g} ({} at alpha {:g}, {} slices of {} pixels): risk {:.4f}, "
                               "unscaled {}".format(cal.scale, cal.bound, cal.alpha, cal.n_slices, cal.n_pixels, cal.risk,
                                                    "n/a" if cal.raw_risk is None else "{:.4f}".format(cal.raw_risk)))
        return cal

    def load_interval_calibration(self, path=None):
        """Read an IntervalCalibration back from `path` (None: `<results_folder>/interval_calibration.json`) into
        `self.interval_calibration`, and return it."""
        import json
        with open(path or os.path.join(self.results_folder, self.INTERVAL_CALIBRATION_FILE)) as f:
            d = json.load(f)
        missing = [k for k in IntervalCalibration._fields if k not in d]
        if missing:
            raise RuntimeError(f"Trainer.load_interval_calibration: the file lacks {missing}")
        self.interval_calibration = IntervalCalibration(**{k: d[k] for k in IntervalCalibration._fields})
        return self.interval_calibration
