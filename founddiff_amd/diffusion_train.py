"""One training step of the reference's residual diffusion around a trainable U-Net (founddiff_amd.unet_train), on HIP kernels
(csrc/fd_train_step.hip): everything between a batch and the U-Net, and between the gradients and the next weights
(src/DADiff.py:1382-1499 ResidualDiffusion.forward / q_sample / p_losses, 1689-1725 the loop body of Trainer.train).

    q_sample(x_start, x_input, t, schedule, ...)   normalize, x_res, q_sample, the cat and the two time inputs: one launch; the noise
                                                   is given, or keyed per slice as the samplers' (fd_keyed_normal's bits)
    residual_loss(pred, target, loss_type, scale)  F.l1_loss / F.mse_loss(reduction='none') -> per-slice mean -> batch mean, with its
                                                   gradient from the same pass (an autograd function)
    p_losses_fn(model_fn, imgs, t, schedule, ...)  p_losses on a free function model_fn(x_in, [time0, time1]) -> list of (B, 1, H, W)
    p_losses(self, imgs, t, ...)                   the same on the reference's attribute names
    ClipAdamEMA(params, ema_params, ...)           clip_grad_norm_ + torch.optim.Adam + zero_grad + the EMA update: three launches
    ClipRAdamEMA(params, ema_params, ...)          the same around torch.optim.RAdam's rule: the reference's optimiser of two U-Nets,
                                                   one object over the parameters of both (joint clip, both updates, one EMA)
    train_step(diffusion_or_fn, opt, batch, ...)   p_losses -> backward per loss -> opt.step()
    GradReducer(opt, group)                        data-parallel training: per micro-batch pack the gradients, all-gather, add the
                                                   ranks' rows in rank order (csrc/fd_grad_sum.hip); train_step(reducer=...) is then
                                                   bit for bit the single process over all ranks' micro-batches
    StoreBatch(store, indices, codes)              a micro-batch that stays in a data.DeviceSliceStore: accepted wherever
                                                   [x_start, x_input] is; q_sample then gathers, flips / rotates and diffuses it in
                                                   one launch (csrc/fd_train_data.hip), fed by one int64 table from pinned memory;
                                                   with windows and crop it is cut to patches in that launch (csrc/fd_train_crop.hip)
    val_items(pred, target, loss_type, ...)        per slice, without a gradient: the loss and the one-step denoising error of a
                                                   model output (csrc/fd_validate.hip); val_draws keys the t and the noise of a
                                                   held-out evaluation per (item, noise band), val_summary reduces the rows per
                                                   band on the host (ResidualDiffusion.eval_items, Trainer.validate)
    structural_loss(out, x_start, x_input, ...)    1 - SSIM of the one-step estimate against x_start (the unclamped map) with its
                                                   gradient from the same call (csrc/fd_ssim_train.hip); ssim_items the per-slice
                                                   means; p_losses_fn(ssim_weight=w) adds it onto the loss and the gradient of the
                                                   row that predicts the residual or x0, inside that row's one autograd node;
                                                   onestep_pair writes the image pair validation measures SSIM on

Binding for a training run:

    import DADiff, founddiff_amd.diffusion_train as dt
    DADiff.ResidualDiffusion.p_losses = dt.p_losses

Deterministic: no float atomics, fixed summation orders that depend on a tensor's own size only, no host synchronisation (the clip
coefficient, the non-finite flag and Adam's step counts stay on the device).  There is no CPU path.

The EMA schedule (ema_schedule) restates ema-pytorch as the reference constructs it (src/DADiff.py:1607).  ema_pytorch is not
available where this project is tested, so that parity is UNPINNED: no test compares it with the package itself.

The checkpoint of DADiff.Trainer.save (checkpoint_pack / checkpoint_unpack) has the reference's five keys; whether its 'opt0' and
'ema' entries load into torch.optim.Adam and ema-pytorch as the reference holds them, and theirs here, is UNPINNED for the same
reason: no test reads a file written by either.

chunk_table, ema_schedule, adam_state_unpack, adam_state_pack, train_batch_indices, train_t_and_seeds, train_augment,
augment_source_index, train_crop, crop_source_index, checkpoint_pack, checkpoint_unpack, check_bands, val_draws and val_summary are
pure host code, and so are radam_scalars, optimizer_kind, checkpoint_pack2 and checkpoint_unpack2: the checkpoint of two U-Nets has
the reference's six keys (CHECKPOINT_KEYS_2), 'opt0' and 'opt1' in torch.optim.RAdam's layout, which the tests load into
torch.optim.RAdam itself.
"""
import numpy as np
import torch

from . import _lib as L
from . import objectives
from ._train import empty, ptr, stream, workspace
from .data import check_batch, crop_pads, crop_pair, upload_table, window_rows

__all__ = ["q_sample", "residual_loss", "p_losses_fn", "p_losses", "ClipAdamEMA", "train_step", "chunk_table", "ema_schedule",
           "adam_state_unpack", "adam_state_pack", "train_batch_indices", "train_t_and_seeds", "train_augment", "augment_source_index",
           "train_crop", "crop_source_index", "StoreBatch", "checkpoint_pack", "checkpoint_unpack", "CHUNK", "check_bands", "val_draws",
           "val_items", "val_summary", "ClipRAdamEMA", "radam_scalars", "optimizer_kind", "CHECKPOINT_KEYS", "CHECKPOINT_KEYS_2",
           "checkpoint_pack2", "checkpoint_unpack2", "GradReducer", "ordered_sum", "dp_micro", "structural_loss", "ssim_items", "onestep_pair",
           "check_ssim_weight"]

CHUNK = 4096                      # elements of a parameter per workgroup (fd_opt_chunk_elems())
_LOSS_TYPES = {"l1": 1, "l2": 2}


# ---- pure host code ----------------------------------------------------------------------------------------------------------------
def chunk_table(numels):
    """(nchunk, 3) int64 = (tensor index, offset, length): every tensor cut into chunks of CHUNK elements from its own start, in
    tensor order.  A tensor's chunks depend on its numel alone."""
    rows = []
    for i, n in enumerate(numels):
        n = int(n)
        if n < 1:
            raise RuntimeError(f"chunk_table: tensor {i} has no elements")
        rows += [(i, off, min(CHUNK, n - off)) for off in range(0, n, CHUNK)]
    return np.asarray(rows, dtype=np.int64).reshape(-1, 3)


def ema_schedule(s0, copied, beta=0.995, update_every=10, update_after_step=100, inv_gamma=1.0, power=2 / 3, min_value=0.0):
    """(mode, decay) of the EMA on the call whose counter value is s0 (0 on the first call); copied: whether the EMA has ever been
    written.  mode 0: nothing; 1: ema = p; 2: ema -= (1 - decay)(ema - p)."""
    if s0 % update_every != 0:
        return 0, 0.0
    if s0 <= update_after_step or not copied:        # a first copy followed by the decayed update of equal tensors is the copy
        return 1, 0.0
    epoch = max(s0 + 1 - update_after_step - 1, 0)
    if epoch <= 0:
        return 2, 0.0
    return 2, min(max(1 - (1 + epoch / inv_gamma) ** -power, min_value), beta)


def adam_state_unpack(sd, n):
    """torch.optim.Adam's state_dict (one param group of n parameters) -> (steps, exp_avg, exp_avg_sq): three lists of length n,
    step counts as ints; a parameter without state has step 0 and None twice."""
    groups = sd["param_groups"]
    if len(groups) != 1 or len(groups[0]["params"]) != n:
        raise RuntimeError(f"load_state_dict: expected one param group of {n} parameters (got {len(groups)} group(s) of "
                           f"{[len(g['params']) for g in groups]})")
    steps, m, v = [0] * n, [None] * n, [None] * n
    for i, key in enumerate(groups[0]["params"]):
        st = sd["state"].get(key)
        if st is None:
            continue
        steps[i], m[i], v[i] = int(round(float(st["step"]))), st["exp_avg"], st["exp_avg_sq"]
    return steps, m, v


def adam_state_pack(steps, exp_avg, exp_avg_sq, group):
    """the inverse: torch.optim.Adam's layout, state[i] = {step, exp_avg, exp_avg_sq} for every parameter that has taken a step;
    group: the hyperparameters of the one param group (its "params" is replaced).  torch.optim.RAdam keeps the same three
    entries per parameter: with its group this is RAdam's layout."""
    state = {i: {"step": torch.tensor(float(s)), "exp_avg": exp_avg[i], "exp_avg_sq": exp_avg_sq[i]}
             for i, s in enumerate(steps) if s > 0}
    return {"state": state, "param_groups": [dict(group, params=list(range(len(steps))))]}


def radam_scalars(step, lr, beta1, beta2):
    """(rectified, step_size, factor) of torch.optim.RAdam (_single_tensor_radam, not capturable) for a tensor at step count
    `step` >= 1, in Python floats (doubles), as lane 0 of a workgroup of fd_opt_radam_ema_f32 computes them:

        bc1 = 1 - beta1^s, bc2 = 1 - beta2^s, rho_inf = 2 / (1 - beta2) - 1, rho = rho_inf - 2 s beta2^s / bc2
        step_size = lr / bc1
        rho > 5:  factor = sqrt((rho - 4)(rho - 2) rho_inf / ((rho_inf - 4)(rho_inf - 2) rho)) sqrt(bc2),
                  p -= step_size factor m / (sqrt(v) + eps)          (eps joins sqrt(v) uncorrected: not Adam's denominator)
        else:     factor = 1,  p -= step_size m

    The kernel rounds step_size * factor to float once.  rho <= rho_inf, so with rho_inf <= 5 (beta2 <= 2 / 3) no step is
    rectified and nothing is divided by rho_inf - 4."""
    s = int(step)
    if s < 1 or not 0 <= beta1 < 1 or not 0 <= beta2 < 1:
        raise RuntimeError(f"radam_scalars: invalid arguments step={step} beta1={beta1} beta2={beta2} (step >= 1, betas in [0, 1))")
    b2s = float(beta2) ** s
    bc1, bc2 = 1.0 - float(beta1) ** s, 1.0 - b2s
    rho_inf = 2.0 / (1.0 - float(beta2)) - 1.0
    rho = rho_inf - 2.0 * s * b2s / bc2
    if rho > 5.0:
        r = ((rho - 4.0) * (rho - 2.0) * rho_inf / ((rho_inf - 4.0) * (rho_inf - 2.0) * rho)) ** 0.5
        return True, float(lr) / bc1, r * bc2 ** 0.5
    return False, float(lr) / bc1, 1.0


def optimizer_kind(group):
    """'adam' or 'radam' for a param group of a state dict, None for neither: torch.optim.Adam's groups carry amsgrad,
    torch.optim.RAdam's decoupled_weight_decay and no amsgrad"""
    if "amsgrad" in group:
        return "adam"
    return "radam" if "decoupled_weight_decay" in group else None


def _check_kind(fn, entry, sd, want):
    """`sd` (the state dict under `entry`) was written by the optimiser `want` ('adam', 'radam'; None: not checked)"""
    if want is None:
        return
    got = [optimizer_kind(g) for g in sd["param_groups"]]
    if any(k != want for k in got):
        names = {"adam": "torch.optim.Adam (ClipAdamEMA)", "radam": "torch.optim.RAdam (ClipRAdamEMA)", None: "an unknown optimiser"}
        raise RuntimeError(f"{fn}: '{entry}' was written by {names[got[0]]}, this run uses {names[want]}: Adam and RAdam state do "
                           f"not load into each other")


# What Trainer.train draws is a pure function of (seed, step, micro-batch): no generator state lives in a checkpoint, and a run resumed
# from one continues as the uninterrupted run would.
_M64 = (1 << 64) - 1


def _mix64(*words):
    """splitmix64 folded over the words: a fixed 64-bit hash in plain integer arithmetic"""
    h = 0x9E3779B97F4A7C15
    for w in words:
        h = (h ^ (int(w) & _M64)) & _M64
        h = (h + 0x9E3779B97F4A7C15) & _M64
        h = ((h ^ (h >> 30)) * 0xBF58476D1CE4E5B9) & _M64
        h = ((h ^ (h >> 27)) * 0x94D049BB133111EB) & _M64
        h ^= h >> 31
    return h


def train_batch_indices(seed, step, micro, batch_size, n, accumulate=1):
    """The dataset indices of micro-batch `micro` of step `step`: sample number k = (step accumulate + micro) batch_size + i is item
    perm_e[k % n] of epoch e = k // n, perm_e a permutation of range(n) keyed by (seed, e).  Every epoch covers the dataset once,
    wherever its ends fall in a batch."""
    if batch_size < 1 or n < 1 or accumulate < 1 or not 0 <= micro < accumulate or step < 0:
        raise RuntimeError(f"train_batch_indices: invalid arguments step={step} micro={micro} batch_size={batch_size} n={n} "
                           f"accumulate={accumulate}")
    k0 = (int(step) * accumulate + micro) * batch_size
    out, perms = [], {}
    for k in range(k0, k0 + batch_size):
        e = k // n
        if e not in perms:
            perms[e] = np.random.default_rng([int(seed) & _M64, e]).permutation(n)
        out.append(int(perms[e][k % n]))
    return out


def train_t_and_seeds(seed, step, micro, indices, num_timesteps):
    """(t, slice_seeds), two int64 arrays, of the items `indices` of micro-batch `micro` of step `step`: t uniform in
    [0, num_timesteps), keyed by (seed, step, micro); a slice's seed by (seed, step, micro, its dataset index), so that its noise
    does not depend on what else is in its batch."""
    t = np.random.default_rng([int(seed) & _M64, int(step), int(micro), 0x74]).integers(0, num_timesteps, len(indices), dtype=np.int64)
    seeds = np.asarray([_mix64(seed, step, micro, i) >> 2 for i in indices], dtype=np.int64)        # 62 bits, as q_sample draws them
    return t, seeds


def train_augment(seed, step, micro, indices, square=True):
    """The flip / rot90 code of every item of `indices` in micro-batch `micro` of step `step`, an int32 array: the low 4 bits of
    _mix64(seed, step, micro, index, 0x61), keyed per item like the slice seeds, so an item's code does not depend on what else
    is in its batch.  Bit 0 flips H, bit 1 flips W, bits 2-3 are k: the item becomes np.rot90(flip_W(flip_H(m)), k, (1, 2)), the
    reference's RandomFlip + RandomRotate90 on a (1, H, W) slice (data/transforms.py:25-82; its flip over the axis of length 1
    is the identity).  The 16 codes are uniform and reach the 8 elements of the dihedral group twice each.  square=False
    clears bit 2: k is 0 or 2, the rotations a non-square slice keeps its shape under."""
    codes = np.asarray([_mix64(seed, step, micro, i, 0x61) & 15 for i in indices], dtype=np.int32)
    return codes if square else codes & ~np.int32(4)


def augment_source_index(code, H, W):
    """(i, j), two (Ho, Wo) integer arrays: output pixel (y, x) of the transform `code` is source pixel (i[y, x], j[y, x]) of the
    (H, W) slice.  The formula the kernels of csrc/fd_train_data.hip implement, in numpy."""
    code = int(code)
    k = (code >> 2) & 3
    if k & 1 and H != W:
        raise RuntimeError(f"augment_source_index: code {code} transposes (k odd), the slice is {H} x {W}")
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    i, j = ((y, x), (x, W - 1 - y), (H - 1 - y, W - 1 - x), (H - 1 - x, y))[k]
    if code & 2:
        j = W - 1 - j
    if code & 1:
        i = H - 1 - i
    return i, j


def train_crop(seed, step, micro, indices, H, W, crop):
    """The crop window (y0, x0) of every item of `indices` in micro-batch `micro` of step `step`, an int64 (len(indices), 2)
    array, for `crop` = an int or (ch, cw) out of (H, W) slices: y0 = _mix64(seed, step, micro, index, 0x63) % max(H - ch, 1),
    x0 = _mix64(seed, step, micro, index, 0x64) % max(W - cw, 1), keyed per item like train_augment, so an item's window does not
    depend on what else is in its batch.  This is the reference's CropToFixed (data/transforms.py:196-249): its
    randint(max_size - crop_size) is uniform over [0, H - ch), so the last possible offset H - ch is never drawn (kept), and its
    randint(1) makes the start 0 when ch >= H (the axis is then taken whole and reflect-padded to ch)."""
    ch, cw = crop_pair("train_crop", crop)
    ny, nx = max(int(H) - ch, 1), max(int(W) - cw, 1)
    out = [(_mix64(seed, step, micro, i, 0x63) % ny, _mix64(seed, step, micro, i, 0x64) % nx) for i in indices]
    return np.asarray(out, dtype=np.int64).reshape(-1, 2)


def crop_source_index(code, y0, x0, H, W, ch, cw):
    """(i, j), two (ch, cw) integer arrays: output pixel (y, x) of the window (y0, x0) of a ch x cw crop under the transform `code`
    is source pixel (i[y, x], j[y, x]) of the (H, W) slice.  The crop comes first (an axis no longer than the crop is taken whole
    and reflect-padded, (c - n) // 2 in front and the rest behind, as np.pad(mode="reflect") does: no edge repeat, one
    reflection), then augment_source_index on the crop.  The formula the kernels of csrc/fd_train_crop.hip implement, in numpy."""
    ic, jc = augment_source_index(code, ch, cw)

    def refl(v, n):
        return np.where(v < 0, -v, np.where(v >= n, 2 * (n - 1) - v, v))
    return refl(y0 + ic - crop_pads(H, ch)[0], H), refl(x0 + jc - crop_pads(W, cw)[0], W)


# What Trainer.validate draws is a pure function of (val_seed, dataset index, band): the same items meet the same t and the same
# noise at every validation of every run, so two numbers differ by the weights alone.
def check_bands(fn, bands, num_timesteps):
    """`bands` as a tuple of ints: at least two strictly increasing edges inside [0, num_timesteps]"""
    is_int = lambda v: isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))
    if not isinstance(bands, (tuple, list)) or len(bands) < 2 or not all(is_int(v) for v in bands):
        raise RuntimeError(f"{fn}: bands must be a tuple of at least two integer edges (got {bands!r})")
    edges = tuple(int(v) for v in bands)
    if any(hi <= lo for lo, hi in zip(edges, edges[1:])) or edges[0] < 0 or edges[-1] > int(num_timesteps):
        raise RuntimeError(f"{fn}: the band edges {edges} must increase strictly inside [0, {int(num_timesteps)}]")
    return edges


def val_draws(val_seed, indices, bands, num_timesteps):
    """(item, band, t, slice_seeds), four int64 arrays with one row per (item, band) pair, items outer and bands inner, of a
    validation over the dataset items `indices`.  `bands` are increasing edges inside [0, num_timesteps]; band k is
    [bands[k], bands[k + 1]): t = bands[k] + _mix64(val_seed, index, k, 0x76) % (bands[k + 1] - bands[k]), the slice's noise seed
    _mix64(val_seed, index, k, 0x6E) >> 2 (62 bits, as q_sample draws them).  Both are functions of (val_seed, index, k) alone:
    not of the training seed, the step, or what else is evaluated with the item."""
    edges = check_bands("val_draws", bands, num_timesteps)
    rows = [(int(i), k, lo + _mix64(val_seed, i, k, 0x76) % (hi - lo), _mix64(val_seed, i, k, 0x6E) >> 2)
            for i in indices for k, (lo, hi) in enumerate(zip(edges, edges[1:]))]
    a = np.asarray(rows, dtype=np.int64).reshape(-1, 4)
    return a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy(), a[:, 3].copy()


def val_summary(items, band, n_bands):
    """The rows of val_items gathered on the host, (n, 2) = (loss, one-step MSE in [0, 1] units) with their band indices (n,),
    per band in float64: {"loss": mean loss, "mse": mean MSE, "psnr": mean of -10 log10(mse), "rmse": mean of sqrt(mse), "n": the
    item count}, lists of n_bands.  PSNR and RMSE are averaged over items, as the reference averages its per-slice metrics
    (src/DADiff.py:1883-1886, 1952).  A band without items has n = 0 and NaN means; NaN rows (no residual output) give NaN.
    Rows of eval_items(ssim=True), (n, 3) with the one-step SSIM as their third column, give "ssim" too: its mean over items."""
    it, bd = np.asarray(items, dtype=np.float64), np.asarray(band)
    if it.ndim != 2 or it.shape[1] not in (2, 3) or bd.shape != (it.shape[0],) or bd.dtype.kind not in "iu" or int(n_bands) < 1:
        raise RuntimeError(f"val_summary: inconsistent shapes items{it.shape} band{bd.shape} (items (n, 2), band (n,) integers, "
                           f"n_bands >= 1)")
    if bd.size and (bd.min() < 0 or bd.max() >= n_bands):
        raise RuntimeError(f"val_summary: band {int(bd[(bd < 0) | (bd >= n_bands)][0])} outside [0, {int(n_bands)})")
    names = ("loss", "mse", "psnr", "rmse") + (("ssim",) if it.shape[1] == 3 else ())
    out = {name: [] for name in names + ("n",)}
    mean = lambda v: float(v.sum() / v.size) if v.size else float("nan")
    for k in range(int(n_bands)):
        rows = it[bd == k]
        with np.errstate(divide="ignore", invalid="ignore"):
            cols = (rows[:, 0], rows[:, 1], -10.0 * np.log10(rows[:, 1]), np.sqrt(rows[:, 1])) + tuple(rows[:, 2:].T)
        for name, v in zip(names, cols):
            out[name].append(mean(v))
        out["n"].append(int(rows.shape[0]))
    return out


CHECKPOINT_KEYS = ("step", "model", "opt0", "ema", "scaler")


def checkpoint_pack(step, model_sd, ema_model_sd, opt_sd, trainable_index, n_params):
    """The dictionary of Trainer.save (src/DADiff.py:1626-1646): {'step', 'model', 'opt0', 'ema', 'scaler': None}.  opt_sd is
    ClipAdamEMA.state_dict() over the trainable parameters; trainable_index[j] is the place of its parameter j in
    diffusion.parameters(), n_params their number: 'opt0' has torch.optim.Adam's layout over ALL of them, the frozen ones (and
    any that never took a step) without state.  'ema' holds ema_model.<key>, initted and step, as ema-pytorch names them."""
    nt = len(trainable_index)
    steps, m, v = adam_state_unpack(opt_sd, nt)
    S, M, V = [0] * n_params, [None] * n_params, [None] * n_params
    for j, i in enumerate(trainable_index):
        S[i], M[i], V[i] = steps[j], m[j], v[j]
    group = {k: val for k, val in opt_sd["param_groups"][0].items() if k != "params"}
    ema = {"ema_model." + k: val for k, val in ema_model_sd.items()}
    ema["initted"] = torch.tensor([bool(opt_sd.get("ema_copied", False))])
    ema["step"] = torch.tensor([int(opt_sd.get("ema_step", 0))])
    return {"step": int(step), "model": model_sd, "opt0": adam_state_pack(S, M, V, group), "ema": ema, "scaler": None}


def checkpoint_unpack(data, trainable_index, n_params, optimizer=None):
    """the inverse: (step, model_sd, ema_model_sd, opt_sd) with opt_sd as ClipAdamEMA.load_state_dict takes it.  optimizer
    ('adam' or 'radam'; None: not checked): the optimiser 'opt0' must have been written by (optimizer_kind)."""
    if set(data) != set(CHECKPOINT_KEYS):
        raise RuntimeError(f"checkpoint_unpack: expected the keys {CHECKPOINT_KEYS} (got {sorted(data)})")
    _check_kind("checkpoint_unpack", "opt0", data["opt0"], optimizer)
    S, M, V = adam_state_unpack(data["opt0"], n_params)
    frozen = set(range(n_params)) - set(trainable_index)
    if any(S[i] for i in frozen):
        raise RuntimeError("checkpoint_unpack: 'opt0' holds state for a frozen parameter")
    group = {k: val for k, val in data["opt0"]["param_groups"][0].items() if k != "params"}
    opt_sd = adam_state_pack([S[i] for i in trainable_index], [M[i] for i in trainable_index], [V[i] for i in trainable_index], group)
    ema = data["ema"]
    opt_sd["ema_step"], opt_sd["ema_copied"] = int(ema["step"].reshape(-1)[0]), bool(ema["initted"].reshape(-1)[0])
    ema_model_sd = {k[len("ema_model."):]: val for k, val in ema.items() if k.startswith("ema_model.")}
    return int(data["step"]), data["model"], ema_model_sd, opt_sd


CHECKPOINT_KEYS_2 = ("step", "model", "opt0", "opt1", "ema", "scaler")


def _unet_places(fn, trainable_index, unet_index):
    """(u, k) per trainable parameter: it is parameter k of U-Net u"""
    if len(unet_index) != 2:
        raise RuntimeError(f"{fn}: unet_index must hold the places of unet0's and of unet1's parameters (got {len(unet_index)} lists)")
    where = {}
    for u, places in enumerate(unet_index):
        for k, i in enumerate(places):
            if i in where:
                raise RuntimeError(f"{fn}: parameter {i} is listed twice in unet_index")
            where[i] = (u, k)
    missing = [i for i in trainable_index if i not in where]
    if missing:
        raise RuntimeError(f"{fn}: trainable parameter {missing[0]} belongs to neither U-Net")
    return [where[i] for i in trainable_index]


def checkpoint_pack2(step, model_sd, ema_model_sd, opt_sd, trainable_index, unet_index):
    """The dictionary of Trainer.save for two U-Nets (src/DADiff.py:1637-1645): CHECKPOINT_KEYS_2.  opt_sd is
    ClipRAdamEMA.state_dict() of the ONE optimiser over the trainable parameters of both U-Nets; trainable_index[j] is the place
    of its parameter j in diffusion.parameters(), unet_index = (the places of unet0.parameters(), those of unet1.parameters()),
    each in that U-Net's own order.  'opt0' has torch.optim.RAdam's layout over unet0.parameters(), 'opt1' over
    unet1.parameters(), as the reference's two optimisers write them; frozen parameters and any that never took a step carry no
    state.  'ema' as checkpoint_pack writes it: the reference keeps one EMA of the whole model."""
    fn = "checkpoint_pack2"
    _check_kind(fn, "opt_sd", opt_sd, "radam")
    steps, m, v = adam_state_unpack(opt_sd, len(trainable_index))
    sizes = [len(places) for places in unet_index]
    S, M, V = ([[0] * n for n in sizes], [[None] * n for n in sizes], [[None] * n for n in sizes])
    for j, (u, k) in enumerate(_unet_places(fn, trainable_index, unet_index)):
        S[u][k], M[u][k], V[u][k] = steps[j], m[j], v[j]
    group = {k: val for k, val in opt_sd["param_groups"][0].items() if k != "params"}
    ema = {"ema_model." + k: val for k, val in ema_model_sd.items()}
    ema["initted"] = torch.tensor([bool(opt_sd.get("ema_copied", False))])
    ema["step"] = torch.tensor([int(opt_sd.get("ema_step", 0))])
    return {"step": int(step), "model": model_sd, "opt0": adam_state_pack(S[0], M[0], V[0], group),
            "opt1": adam_state_pack(S[1], M[1], V[1], group), "ema": ema, "scaler": None}


def checkpoint_unpack2(data, trainable_index, unet_index):
    """the inverse: (step, model_sd, ema_model_sd, opt_sd) with opt_sd as ClipRAdamEMA.load_state_dict takes it, over the
    trainable parameters of both U-Nets in trainable_index's order.  The hyperparameters are 'opt0''s."""
    fn = "checkpoint_unpack2"
    if set(data) != set(CHECKPOINT_KEYS_2):
        raise RuntimeError(f"{fn}: expected the keys {CHECKPOINT_KEYS_2} (got {sorted(data)})")
    places = _unet_places(fn, trainable_index, unet_index)
    S, M, V = [], [], []
    for u, entry in enumerate(("opt0", "opt1")):
        _check_kind(fn, entry, data[entry], "radam")
        s, m, v = adam_state_unpack(data[entry], len(unet_index[u]))
        S.append(s), M.append(m), V.append(v)
    live = set(places)
    if any(S[u][k] for u in range(2) for k in range(len(S[u])) if (u, k) not in live):
        raise RuntimeError(f"{fn}: 'opt0' or 'opt1' holds state for a frozen parameter")
    group = {k: val for k, val in data["opt0"]["param_groups"][0].items() if k != "params"}
    opt_sd = adam_state_pack([S[u][k] for u, k in places], [M[u][k] for u, k in places], [V[u][k] for u, k in places], group)
    ema = data["ema"]
    opt_sd["ema_step"], opt_sd["ema_copied"] = int(ema["step"].reshape(-1)[0]), bool(ema["initted"].reshape(-1)[0])
    ema_model_sd = {k[len("ema_model."):]: val for k, val in ema.items() if k.startswith("ema_model.")}
    return int(data["step"]), data["model"], ema_model_sd, opt_sd


# ---- argument checks: types and dtypes, then shapes, then devices, before anything launches ------------------------------------------
def _check_f32(fn, named, optional=()):
    for name, v in named:
        if v is None and name in optional:
            continue
        if not isinstance(v, torch.Tensor):
            raise RuntimeError(f"{fn}: {name} must be a tensor (got {type(v).__name__})")
        if v.dtype != torch.float32:
            raise RuntimeError(f"{fn}: {name} must be float32 (got {v.dtype})")


def _check_i64(fn, name, v):
    if not isinstance(v, torch.Tensor):
        raise RuntimeError(f"{fn}: {name} must be a tensor (got {type(v).__name__})")
    if v.dtype != torch.int64:
        raise RuntimeError(f"{fn}: {name} must be int64 (got {v.dtype})")


def _check_gpu(fn, named):
    first = None
    for name, v in named:
        if v is None:
            continue
        if not v.is_cuda:
            raise RuntimeError(f"{fn}: {name} must live on the GPU (there is no CPU path)")
        if first is None:
            first = (name, v.device)
        elif v.device != first[1]:
            raise RuntimeError(f"{fn}: {name} lives on {v.device}, {first[0]} on {first[1]}")


_TABLES = {}      # (ids of the host tables, device) -> (the host tables, their copies on the device)


def _schedule_tables(fn, schedule):
    if not isinstance(schedule, dict) or "alphas_cumsum" not in schedule or "betas_cumsum" not in schedule:
        raise RuntimeError(f"{fn}: schedule must be a dict with alphas_cumsum and betas_cumsum (DADiff.residual_schedule(T))")
    ac, bc = schedule["alphas_cumsum"], schedule["betas_cumsum"]
    _check_f32(fn, (("schedule['alphas_cumsum']", ac), ("schedule['betas_cumsum']", bc)))
    if ac.dim() != 1 or ac.shape != bc.shape or ac.numel() < 1:
        raise RuntimeError(f"{fn}: inconsistent shapes alphas_cumsum{tuple(ac.shape)} betas_cumsum{tuple(bc.shape)} (both (T,))")
    return ac, bc


def _upload_tables(ac, bc, dev):
    """the two tables on dev, uploaded once per schedule"""
    if ac.device == dev and bc.device == dev:
        return ac.contiguous(), bc.contiguous()
    key = (id(ac), id(bc), dev)
    if key not in _TABLES:
        _TABLES[key] = (ac, bc, ac.to(dev).contiguous(), bc.to(dev).contiguous())      # keeps ac, bc alive: the ids stay theirs
    return _TABLES[key][2:]


def _check_qsample(fn, x_start, x_input, t, schedule, noise, slice_seeds, dims=(2, 4)):
    _check_f32(fn, (("x_start", x_start), ("x_input", x_input), ("noise", noise)), optional=("noise",))
    _check_i64(fn, "t", t)
    if slice_seeds is not None:
        _check_i64(fn, "slice_seeds", slice_seeds)
    if noise is not None and slice_seeds is not None:
        raise RuntimeError(f"{fn}: give either noise or slice_seeds, not both")
    ac, bc = _schedule_tables(fn, schedule)
    shapes = " ".join(f"{n}{tuple(v.shape)}" for n, v in (("x_start", x_start), ("x_input", x_input), ("t", t), ("noise", noise),
                                                         ("slice_seeds", slice_seeds)) if v is not None)
    if x_start.dim() not in dims or x_start.numel() < 1 or (x_start.dim() == 4 and x_start.shape[1] != 1):
        raise RuntimeError(f"{fn}: unsupported shape {shapes} (x_start is (B, 1, H, W)" + (" or (B, npix))" if 2 in dims else ")"))
    B = x_start.shape[0]
    if x_input.shape != x_start.shape or tuple(t.shape) != (B,) or (noise is not None and noise.shape != x_start.shape) or \
            (slice_seeds is not None and tuple(slice_seeds.shape) != (B,)):
        raise RuntimeError(f"{fn}: inconsistent shapes {shapes} (x_input and noise as x_start, t and slice_seeds (B,))")
    if B > 65535:
        raise RuntimeError(f"{fn}: unsupported shape {shapes} (at most 65535 slices)")
    _check_gpu(fn, (("x_start", x_start), ("x_input", x_input), ("t", t), ("noise", noise), ("slice_seeds", slice_seeds)))
    return ac, bc


class StoreBatch:
    """Items `indices` of a data.DeviceSliceStore under the transform `codes` (train_augment; None: as stored): a micro-batch
    that is never assembled.  Accepted wherever [x_start, x_input] is (q_sample, p_losses_fn, p_losses, train_step,
    ResidualDiffusion.forward / p_losses); the images are the store's, in [0, 1].  With `crop` (an int or (h, w)) every item is
    first cut to the window of `windows` ((B, 2) = (y0, x0) per item, train_crop; None: zeros) and the codes apply to the crop
    (DeviceSliceStore.batch has the rules); the batch is then (B, 1, h, w).  Everything is checked here: types, shapes, then the
    ranges of the indices, the codes and the windows."""

    def __init__(self, store, indices, codes=None, windows=None, crop=None):
        self.indices, self.codes, self.windows, self.crop = check_batch("StoreBatch", store, indices, codes, windows, crop)
        self.store = store

    def __len__(self):
        return len(self.indices)

    @property
    def device(self):
        return self.store.device

    @property
    def shape(self):
        return (len(self.indices), 1) + ((self.store.H, self.store.W) if self.crop is None else self.crop)


def _check_qsample_store(fn, sb, t, schedule, noise, slice_seeds):
    """t and slice_seeds may stay on the host (a sequence, an array or a CPU tensor of integers: they travel in the batch's table)
    or be int64 tensors on the store's device.  Returns (ac, bc, t, slice_seeds), the host ones as int64 arrays."""
    B = len(sb)

    def ints(name, v):
        if isinstance(v, torch.Tensor) and v.is_cuda:
            _check_i64(fn, name, v)
            return v
        a = v.detach().numpy() if isinstance(v, torch.Tensor) else (np.asarray(v) if isinstance(v, (list, tuple, np.ndarray)) else None)
        if a is None:
            raise RuntimeError(f"{fn}: {name} must be a tensor or a sequence of integers (got {type(v).__name__})")
        if a.dtype.kind not in "iu":
            raise RuntimeError(f"{fn}: {name} must be int64 (got {a.dtype})")
        return a.astype(np.int64)
    _check_f32(fn, (("noise", noise),), optional=("noise",))
    t = ints("t", t)
    if slice_seeds is not None:
        slice_seeds = ints("slice_seeds", slice_seeds)
    if noise is not None and slice_seeds is not None:
        raise RuntimeError(f"{fn}: give either noise or slice_seeds, not both")
    ac, bc = _schedule_tables(fn, schedule)
    shapes = " ".join(f"{n}{tuple(v.shape)}" for n, v in (("batch", sb), ("t", t), ("noise", noise), ("slice_seeds", slice_seeds))
                      if v is not None)
    if tuple(t.shape) != (B,) or (noise is not None and tuple(noise.shape) != sb.shape) or \
            (slice_seeds is not None and tuple(slice_seeds.shape) != (B,)):
        raise RuntimeError(f"{fn}: inconsistent shapes {shapes} (noise as the batch, t and slice_seeds (B,))")
    for name, v in (("t", t), ("noise", noise), ("slice_seeds", slice_seeds)):
        if isinstance(v, torch.Tensor) and v.device != sb.device:
            raise RuntimeError(f"{fn}: {name} lives on {v.device}, the store on {sb.device}")
    return ac, bc, t, slice_seeds


def _q_sample_store(sb, t, schedule, noise, slice_seeds, step, normalize, x0_out):
    fn = "q_sample"
    ac, bc, t, slice_seeds = _check_qsample_store(fn, sb, t, schedule, noise, slice_seeds)
    st, dev, B = sb.store, sb.device, len(sb)
    with torch.no_grad(), torch.cuda.device(dev):
        ac, bc = _upload_tables(ac, bc, dev)
        if noise is None and slice_seeds is None:
            slice_seeds = torch.randint(0, 1 << 62, (B,), device=dev, dtype=torch.int64)
        # one table: the NDCT slots, the indices, then whichever of the codes, t and the seeds are on the host, then the windows
        # (two rows: side by side the (B, 2) array)
        rows, at = [st.nd_index[sb.indices], sb.indices], {}
        for name, v in (("codes", sb.codes), ("t", t), ("seeds", slice_seeds)):
            if isinstance(v, np.ndarray):
                at[name] = len(rows)
                rows.append(v)
        if sb.windows is not None:
            at["windows"] = len(rows)
            rows += window_rows(sb.windows)
        tab = upload_table(rows, dev)
        col = lambda name, v: tab[at[name]] if name in at else (None if v is None else v.contiguous())
        codes, tt, seeds = col("codes", sb.codes), col("t", t), col("seeds", slice_seeds)
        new = empty(dev)
        x_in, x_res, times = new((B, 2) + sb.shape[2:]), new(sb.shape), new(2, B)
        x0 = new(sb.shape) if x0_out else None
        if noise is None:
            nz, out = None, new(sb.shape)
        else:
            nz, out = noise.detach().contiguous(), None
        if sb.crop is None:
            L.call("fd_res_qsample_store_f32", ptr(st.nd), ptr(st.ld), st.n_nd, st.n_ld, ptr(tab[0]), ptr(tab[1]), ptr(codes), ptr(tt),
                   ptr(ac), ptr(bc), ac.numel(), ptr(nz), ptr(seeds), int(step) & 0x7FFFFFFF, int(bool(normalize)), ptr(x_in),
                   ptr(x_res), ptr(out), ptr(times), ptr(x0), B, st.H, st.W, stream(dev))
        else:
            L.call("fd_res_qsample_crop_f32", ptr(st.nd), ptr(st.ld), st.n_nd, st.n_ld, ptr(tab[0]), ptr(tab[1]), ptr(codes),
                   ptr(col("windows", None)), ptr(tt), ptr(ac), ptr(bc), ac.numel(), ptr(nz), ptr(seeds), int(step) & 0x7FFFFFFF,
                   int(bool(normalize)), ptr(x_in), ptr(x_res), ptr(out), ptr(times), ptr(x0), B, st.H, st.W, sb.crop[0], sb.crop[1],
                   stream(dev))
    res = (x_in, x_res, (noise if out is None else out), times)
    return res + (x0,) if x0_out else res


def q_sample(x_start, x_input, t, schedule, noise=None, slice_seeds=None, step=0, normalize=True, x0_out=False):
    """ResidualDiffusion.forward's normalize + p_losses' x_res, q_sample and cat (src/DADiff.py:1382-1388, 1412-1440, 1493-1497).
    x_start, x_input (B, 1, H, W) or (B, npix) fp32, in [0, 1] with normalize=True (2x - 1 is applied to both); t (B,) int64;
    schedule = DADiff.residual_schedule(T) (its alphas_cumsum and betas_cumsum are uploaded once).  noise as x_start, or
    slice_seeds (B,) int64: the noise of slice b is then fd_keyed_normal's stream of (slice_seeds[b], step), whatever its batch or
    rank.  With neither, the seeds are drawn from torch's generator of the device.
    Returns x_in (B, 2, ...) = cat(x_t, x_input), x_res = x_input - x_start, the noise, times (2, B) = alphas_cumsum[t] T,
    betas_cumsum[t] T; with x0_out a fifth result, the normalised x_start (pred_x0_noise's target).  Nothing is differentiable.
    x_start may be a StoreBatch (x_input is then None): the gather, the flip / rot90 of its codes and all of the above are one
    launch of fd_res_qsample_store_f32, bit for bit what store.batch() followed by this function gives; t and slice_seeds may
    then stay on the host, and go up with the indices and the codes as one int64 table from pinned memory.  A StoreBatch with a
    crop takes fd_res_qsample_crop_f32 instead: every result is (B, ., h, w), with the bits of store.batch(..., windows, crop)
    followed by this function."""
    fn = "q_sample"
    if isinstance(x_start, StoreBatch):
        if x_input is not None:
            raise RuntimeError(f"{fn}: with a StoreBatch x_input must be None (the batch holds both images)")
        return _q_sample_store(x_start, t, schedule, noise, slice_seeds, step, normalize, x0_out)
    ac, bc = _check_qsample(fn, x_start, x_input, t, schedule, noise, slice_seeds)
    dev = x_start.device
    B = x_start.shape[0]
    npix = x_start.numel() // B
    with torch.no_grad(), torch.cuda.device(dev):
        ac, bc = _upload_tables(ac, bc, dev)
        if noise is None and slice_seeds is None:
            slice_seeds = torch.randint(0, 1 << 62, (B,), device=dev, dtype=torch.int64)
        x0, xi, tt = x_start.detach().contiguous(), x_input.detach().contiguous(), t.contiguous()
        new = empty(dev)
        x_in, x_res, times = new((B, 2) + tuple(x_start.shape[2:] if x_start.dim() == 4 else (npix,))), new(x_start.shape), new(2, B)
        if noise is None:
            nz, out, seeds = None, new(x_start.shape), slice_seeds.contiguous()
        else:
            nz, out, seeds = noise.detach().contiguous(), None, None
        L.call("fd_res_qsample_f32", ptr(x0), ptr(xi), ptr(tt), ptr(ac), ptr(bc), ac.numel(), ptr(nz), ptr(seeds), int(step) & 0x7FFFFFFF,
               int(bool(normalize)), ptr(x_in), ptr(x_res), ptr(out), ptr(times), B, npix, stream(dev))
        res = (x_in, x_res, (noise if out is None else out), times)
        if x0_out:
            xn = x0
            if normalize:
                xn = torch.empty_like(x_res)
                L.call("fd_affine_f32", ptr(x0), 2.0, -1.0, ptr(xn), xn.numel(), stream(dev))
            res += (xn,)
    return res


def _check_loss(fn, pred, target, loss_type, scale):
    _check_f32(fn, (("pred", pred), ("target", target)))
    if loss_type not in _LOSS_TYPES:
        raise RuntimeError(f"{fn}: invalid loss type {loss_type!r} ('l1' or 'l2')")
    if not isinstance(scale, (int, float)):
        raise RuntimeError(f"{fn}: scale must be a number (got {type(scale).__name__})")
    if pred.dim() < 1 or pred.numel() < 1 or pred.shape != target.shape:
        raise RuntimeError(f"{fn}: inconsistent shapes pred{tuple(pred.shape)} target{tuple(target.shape)} (equal, (B, ...))")
    if pred.shape[0] > 65535:
        raise RuntimeError(f"{fn}: unsupported shape pred{tuple(pred.shape)} (at most 65535 slices)")
    _check_gpu(fn, (("pred", pred), ("target", target)))


class _Loss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, loss_type, scale):
        _check_loss("residual_loss", pred, target, loss_type, scale)
        dev = pred.device
        B = pred.shape[0]
        npix = pred.numel() // B
        pf, tf = pred.contiguous(), target.contiguous()
        with torch.cuda.device(dev):
            new = empty(dev)
            loss, dpred = new(1), new(pred.shape)
            ws = workspace("fd_res_loss_ws_floats", dev, B, npix)
            L.call("fd_res_loss_f32", ptr(pf), ptr(tf), _LOSS_TYPES[loss_type], float(scale), ptr(loss), ptr(dpred), ptr(ws), B, npix,
                   stream(dev))
        ctx.save_for_backward(dpred)
        return loss.view(())

    @staticmethod
    def backward(ctx, dloss):
        dpred, = ctx.saved_tensors
        if tuple(dloss.shape) != ():
            raise RuntimeError(f"residual_loss: the gradient of the result must be a scalar (got {tuple(dloss.shape)})")
        dev = dpred.device
        with torch.cuda.device(dev):
            out = torch.empty_like(dpred)
            L.call("fd_scale_dev_f32", ptr(dpred), ptr(dloss.float().contiguous()), ptr(out), dpred.numel(), stream(dev))
        return out, None, None, None


def residual_loss(pred, target, loss_type, scale=1.0):
    """scale * reduce(loss_fn(pred, target, reduction='none'), 'b ... -> b (...)', 'mean').mean() (src/DADiff.py:1476-1481), a
    scalar on the device.  pred, target (B, ...) fp32 of equal shapes; loss_type 'l1' or 'l2'.  Differentiable in pred: the
    gradient comes from the forward pass (sign(0) = 0 for l1, as torch) and the backward multiplies it by the incoming scalar.
    The target gets no gradient."""
    _check_loss("residual_loss", pred, target, loss_type, scale)
    return _Loss.apply(pred, target, loss_type, scale)


# ---- the structural term (csrc/fd_ssim_train.hip) ------------------------------------------------------------------------------------
def check_ssim_weight(fn, w):
    """`w` as a float: a finite number >= 0"""
    if isinstance(w, (bool, np.bool_)) or not isinstance(w, (int, float, np.integer, np.floating)) or not np.isfinite(w) or w < 0:
        raise RuntimeError(f"{fn}: ssim_weight must be a finite number >= 0 (got {w!r})")
    return float(w)


def _check_ssim(fn, out, x_start, x_input, residual, scale):
    """as _check_loss: types and dtypes, then shapes, then devices.  Returns (B, H, W)."""
    _check_f32(fn, (("out", out), ("x_start", x_start), ("x_input", x_input)), optional=() if residual else ("x_input",))
    if not isinstance(scale, (int, float)):
        raise RuntimeError(f"{fn}: scale must be a number (got {type(scale).__name__})")
    named = (("out", out), ("x_start", x_start), ("x_input", x_input if residual else None))
    shapes = " ".join(f"{n}{tuple(v.shape)}" for n, v in named if v is not None)
    if out.dim() not in (3, 4) or out.numel() < 1 or (out.dim() == 4 and out.shape[1] != 1) or \
            any(v is not None and v.shape != out.shape for _, v in named):
        raise RuntimeError(f"{fn}: inconsistent shapes {shapes} (equal, (B, 1, H, W) or (B, H, W))")
    B, (H, W) = out.shape[0], out.shape[-2:]
    if H < 6 or W < 6:
        raise RuntimeError(f"{fn}: unsupported shape {shapes} (the 11-tap window's reflect padding of 5 needs H, W >= 6)")
    if B > 65535 or H > 32768 or W > 32768:
        raise RuntimeError(f"{fn}: unsupported shape {shapes} (at most 65535 slices, H, W <= 32768)")
    _check_gpu(fn, named)
    return B, H, W


def _slices(x, npix):
    """(the tensor to keep alive, its batch stride in elements): x itself where its slices are dense, npix elements each, at a
    common distance -- a channel of q_sample's x_in goes to the kernels as it lies --, else a dense copy"""
    if x.dim() == 4:
        x = x[:, 0]
    if x.stride()[1:] == (x.shape[2], 1) and (x.shape[0] == 1 or x.stride(0) >= npix):
        return x, (x.stride(0) if x.shape[0] > 1 else npix)
    return x.contiguous(), npix


def _ssim_launch(out, x_input, x_start, residual, scale, loss, items, dout, accumulate, dims):
    B, H, W = dims
    dev = out.device
    xi, ld = _slices(x_input.detach(), H * W) if residual else (None, 0)
    ws = workspace("fd_ssim_loss_ws_floats", dev, B, H, W)
    L.call("fd_ssim_loss_f32", ptr(out), ptr(xi), ld, ptr(x_start), int(bool(residual)), float(scale), ptr(loss), ptr(items), ptr(dout),
           int(bool(accumulate)), ptr(ws), B, H, W, stream(dev))


class _RowLoss(torch.autograd.Function):
    """One loss of one model output: loss_type None: the structural term alone (scale); else residual_loss(out, target, loss_type,
    scale) with the structural term under scale * ssim_weight added onto its loss and its gradient in the forward.  The backward
    is _Loss's: the saved gradient times the incoming scalar."""

    @staticmethod
    def forward(ctx, out, target, x_input, x_start, loss_type, scale, residual, ssim_weight):
        dims = _check_ssim("structural_loss", out, x_start, x_input, residual, scale)
        dev, B = out.device, out.shape[0]
        of, x0 = out.contiguous(), x_start.detach().contiguous()
        with torch.cuda.device(dev):
            new = empty(dev)
            loss, dout = new(1), new(out.shape)
            if loss_type is not None:
                npix = out.numel() // B
                ws = workspace("fd_res_loss_ws_floats", dev, B, npix)
                L.call("fd_res_loss_f32", ptr(of), ptr(target.contiguous()), _LOSS_TYPES[loss_type], float(scale), ptr(loss), ptr(dout),
                       ptr(ws), B, npix, stream(dev))
            _ssim_launch(of, x_input, x0, residual, float(scale) * float(ssim_weight), loss, None, dout, loss_type is not None, dims)
        ctx.save_for_backward(dout)
        return loss.view(())

    @staticmethod
    def backward(ctx, dloss):
        return _Loss.backward(ctx, dloss) + (None,) * 4


def structural_loss(out, x_start, x_input=None, *, residual, scale=1.0):
    """scale * (1 - mean over slices of (mean over pixels of S)), a scalar on the device: S the SSIM map of fd_metrics (11-tap
    Gaussian, sigma 1.5, reflect padding of 5, C1 = 0.01^2, C2 = 0.03^2 in [0, 1] units) WITHOUT its clamp to [0, 1], between
    y = (x_start + 1) / 2 and the one-step estimate p = (x_input - out + 1) / 2 of a residual output (residual=True; x_input is
    then required) or p = (out + 1) / 2 of an x0 output; nothing is clamped.  out, x_start, x_input (B, 1, H, W) or (B, H, W) fp32
    in [-1, 1], as q_sample returns them; H, W >= 6.  Differentiable in out alone: the gradient comes from the forward pass
    (csrc/fd_ssim_train.hip) and the backward multiplies it by the incoming scalar, as residual_loss."""
    fn = "structural_loss"
    if not isinstance(residual, (bool, np.bool_)):
        raise RuntimeError(f"{fn}: residual must be a bool (got {residual!r})")
    if residual and x_input is None:
        raise RuntimeError(f"{fn}: a residual output needs x_input (the estimate is x_input - out)")
    _check_ssim(fn, out, x_start, x_input, residual, scale)
    return _RowLoss.apply(out, None, x_input, x_start, None, scale, bool(residual), 1.0)


def ssim_items(out, x_start, x_input=None, *, residual):
    """(B,) on the device, without a gradient: per slice the mean of the unclamped map S of structural_loss, whose value is
    scale * (1 - ssim_items(...).mean()).  A slice's entry does not depend on the rest of its batch."""
    fn = "ssim_items"
    if residual and x_input is None:
        raise RuntimeError(f"{fn}: a residual output needs x_input (the estimate is x_input - out)")
    dims = _check_ssim(fn, out, x_start, x_input, bool(residual), 1.0)
    dev = out.device
    with torch.no_grad(), torch.cuda.device(dev):
        items = empty(dev)(dims[0])
        _ssim_launch(out.detach().contiguous(), x_input, x_start.detach().contiguous(), bool(residual), 1.0, None, items, None, False, dims)
    return items


def onestep_pair(pred, x_input, x_start):
    """(u(clamp(x_input - clamp(pred))), u(x_start)), two tensors shaped as pred in [0, 1] units, from one launch of
    fd_onestep_u01_f32: val_items' one-step estimate as the image pair metrics.compute_metrics reads.  Nothing is differentiable."""
    fn = "onestep_pair"
    named = (("pred", pred), ("x_input", x_input), ("x_start", x_start))
    _check_f32(fn, named)
    if pred.dim() < 2 or pred.numel() < 1 or any(v.shape != pred.shape for _, v in named):
        raise RuntimeError(f"{fn}: inconsistent shapes " + " ".join(f"{n}{tuple(v.shape)}" for n, v in named) + " (equal, (B, ...))")
    if pred.shape[0] > 65535:
        raise RuntimeError(f"{fn}: unsupported shape pred{tuple(pred.shape)} (at most 65535 slices)")
    _check_gpu(fn, named)
    dev, B = pred.device, pred.shape[0]
    npix = pred.numel() // B
    with torch.no_grad(), torch.cuda.device(dev):
        pf, xi, x0 = pred.detach().contiguous(), x_input.detach().contiguous(), x_start.detach().contiguous()
        est, tgt = torch.empty_like(pf), torch.empty_like(pf)
        L.call("fd_onestep_u01_f32", ptr(pf), ptr(xi), npix, ptr(x0), ptr(est), ptr(tgt), B, npix, stream(dev))
    return est, tgt


def val_items(pred, target, loss_type, x_input=None, x_start=None):
    """(B, 2) on the device, one row per slice, from one pass of fd_val_items_f32 (csrc/fd_validate.hip) that writes no gradient:
    column 0 = the slice's mean of |pred - target| ('l1') or (pred - target)^2 ('l2'), so that its mean over the batch is
    residual_loss(pred, target, loss_type); column 1 = the one-step denoising error of a residual output, the mean of
    (u(x0_hat) - u(x_start))^2 with x0_hat = clamp(x_input - clamp(pred, -1, 1), -1, 1) -- the samplers' last step, applied at
    whatever noise level pred was made at -- and u(v) = clamp((v + 1) / 2, 0, 1), the [0, 1] units of compute_psnr / compute_rmse.
    x_input and x_start are the normalised images ([-1, 1], as q_sample returns them), shaped as pred; give both, or neither:
    column 1 is then NaN.  A slice's row does not depend on the rest of its batch.  Nothing is differentiable."""
    fn = "val_items"
    _check_f32(fn, (("pred", pred), ("target", target), ("x_input", x_input), ("x_start", x_start)), optional=("x_input", "x_start"))
    if loss_type not in _LOSS_TYPES:
        raise RuntimeError(f"{fn}: invalid loss type {loss_type!r} ('l1' or 'l2')")
    if (x_input is None) != (x_start is None):
        raise RuntimeError(f"{fn}: give both x_input and x_start, or neither")
    named = (("pred", pred), ("target", target), ("x_input", x_input), ("x_start", x_start))
    if pred.dim() < 1 or pred.numel() < 1 or any(v is not None and v.shape != pred.shape for _, v in named):
        shapes = " ".join(f"{n}{tuple(v.shape)}" for n, v in named if v is not None)
        raise RuntimeError(f"{fn}: inconsistent shapes {shapes} (equal, (B, ...))")
    if pred.shape[0] > 65535:
        raise RuntimeError(f"{fn}: unsupported shape pred{tuple(pred.shape)} (at most 65535 slices)")
    _check_gpu(fn, named)
    dev, B = pred.device, pred.shape[0]
    npix = pred.numel() // B
    with torch.no_grad(), torch.cuda.device(dev):
        pf, tf = pred.detach().contiguous(), target.detach().contiguous()
        xi, x0 = (None, None) if x_input is None else (x_input.detach().contiguous(), x_start.detach().contiguous())
        items = empty(dev)(B, 2)
        ws = workspace("fd_val_items_ws_floats", dev, B, npix)
        L.call("fd_val_items_f32", ptr(pf), ptr(tf), ptr(xi), ptr(x0), _LOSS_TYPES[loss_type], ptr(items), ptr(ws), B, npix, stream(dev))
    return items


def _diffused(fn, imgs, t, schedule, noise, slice_seeds, step, normalize, x0_out):
    """The preamble of p_losses_fn and ResidualDiffusion.eval_items: imgs = [x_start, x_input] or a StoreBatch, checked and put
    through q_sample -> (x_in, the two time inputs, the targets by the names of objectives.TRAINING: "res", "noise" and, with
    x0_out, "x0")."""
    if isinstance(imgs, StoreBatch):
        _check_qsample_store(fn, imgs, t, schedule, noise, slice_seeds)
        pair = (imgs, None)
    else:
        if not isinstance(imgs, (list, tuple)) or len(imgs) != 2:
            raise RuntimeError(f"{fn}: imgs must be [x_start, x_input] (condition=True without an input condition)")
        pair = tuple(imgs)
        _check_qsample(fn, *pair, t, schedule, noise, slice_seeds, dims=(4,))
    x_in, x_res, noise, times, *x0 = q_sample(*pair, t, schedule, noise, slice_seeds, step, normalize, x0_out=x0_out)
    return x_in, times, dict(zip(("res", "noise", "x0"), (x_res, noise, *x0)))


def p_losses_fn(model_fn, imgs, t, schedule, objective="pred_res", loss_type="l1", noise=None, slice_seeds=None, step=0, scale=1.0,
                normalize=False, ssim_weight=0.0):
    """p_losses (src/DADiff.py:1399-1482) for condition=True, input_condition=False on a free function:
    model_fn(x_in (B, 2, H, W), [time0 (B,), time1 (B,)]) -> list of (B, 1, H, W), one per U-Net.  imgs = [x_start, x_input];
    normalize=True takes them in [0, 1] as ResidualDiffusion.forward does.  Returns the list of losses, each times scale.
    ssim_weight > 0 (the reference carries a structural term on the one-step estimate commented out, src/DADiff.py:1480): the
    loss of the row that predicts "res" or "x0" becomes residual_loss + structural_loss(scale=scale * ssim_weight), bit for bit,
    in the loss and in the gradient, from one autograd node; a "noise" row has no term, and an objective without such a row
    ('pred_noise') raises before anything launches.  0.0 is the path without the term: the same launches as ever."""
    fn = "p_losses"
    if not callable(model_fn):
        raise RuntimeError(f"{fn}: model_fn must be callable (got {type(model_fn).__name__})")
    objectives.check_objective(objective, RuntimeError, f"{fn}: ")
    if loss_type not in _LOSS_TYPES:
        raise RuntimeError(f"{fn}: invalid loss type {loss_type!r} ('l1' or 'l2')")
    ssim_weight = check_ssim_weight(fn, ssim_weight)
    rows = objectives.TRAINING[objective]
    if ssim_weight > 0:
        if not any(r.target in ("res", "x0") for r in rows):
            raise RuntimeError(f"{fn}: ssim_weight={ssim_weight} needs an output with a one-step estimate ('res' or 'x0'); objective "
                               f"{objective!r} predicts the noise alone")
        first = imgs if isinstance(imgs, StoreBatch) else (imgs[0] if isinstance(imgs, (list, tuple)) and imgs else None)
        hw = tuple(getattr(first, "shape", ()))[-2:]                     # (anything else is _diffused's to refuse)
        if len(hw) == 2 and min(hw) < 6:
            raise RuntimeError(f"{fn}: ssim_weight={ssim_weight} on images of {hw[0]} x {hw[1]}: the 11-tap window's reflect padding "
                               f"of 5 needs H, W >= 6")
    x_in, times, targets = _diffused(fn, imgs, t, schedule, noise, slice_seeds, step, normalize,
                                     x0_out=ssim_weight > 0 or any(r.target == "x0" for r in rows))
    model_out = model_fn(x_in, [times[0], times[1]])
    target = [targets[r.target] for r in rows]
    if not isinstance(model_out, (list, tuple)) or len(model_out) != len(target):
        raise RuntimeError(f"{fn}: objective {objective!r} needs {len(target)} model output(s) (got "
                           f"{len(model_out) if isinstance(model_out, (list, tuple)) else type(model_out).__name__})")
    if ssim_weight == 0:
        return [residual_loss(o, tg, loss_type, scale) for o, tg in zip(model_out, target)]
    losses = []
    for r, o, tg in zip(rows, model_out, target):
        if r.target == "noise":
            losses.append(residual_loss(o, tg, loss_type, scale))
            continue
        _check_loss("residual_loss", o, tg, loss_type, scale)
        losses.append(_RowLoss.apply(o, tg, x_in[:, 1:2] if r.residual else None, targets["x0"], loss_type, scale, r.residual, ssim_weight))
    return losses


def _diffusion_args(fn, self):
    """the reference's attributes behind p_losses, checked"""
    if getattr(self, "self_condition", False) or getattr(getattr(self, "model", None), "self_condition", False):
        raise RuntimeError(f"{fn}: self_condition is not supported")
    if getattr(self, "input_condition", False):
        raise RuntimeError(f"{fn}: input_condition is not supported")
    if not getattr(self, "condition", True):
        raise RuntimeError(f"{fn}: condition=False (generation) is not supported")
    schedule = dict(alphas_cumsum=self.alphas_cumsum, betas_cumsum=self.betas_cumsum)
    if schedule["alphas_cumsum"].numel() != self.num_timesteps:
        raise RuntimeError(f"{fn}: alphas_cumsum has {schedule['alphas_cumsum'].numel()} rows, num_timesteps is {self.num_timesteps}")
    ssim_weight = check_ssim_weight(fn, getattr(self, "ssim_weight", 0.0))       # reference-shaped objects have none: no term
    return (lambda x, times: self.model(x, times)), schedule, self.objective, self.loss_type, ssim_weight


def p_losses(self, imgs, t, noise=None, slice_seeds=None, step=0, scale=1.0):
    """ResidualDiffusion.p_losses on the reference's attribute names (objective, loss_type, condition, num_timesteps, model, the
    alphas_cumsum / betas_cumsum buffers): imgs = [x_start, x_input] already normalised, as ResidualDiffusion.forward hands them
    over.  self_condition and input_condition raise before anything launches."""
    model_fn, schedule, objective, loss_type, ssim_weight = _diffusion_args("p_losses", self)
    return p_losses_fn(model_fn, imgs, t, schedule, objective, loss_type, noise, slice_seeds, step, scale, normalize=False,
                       ssim_weight=ssim_weight)


# ---- the optimiser -----------------------------------------------------------------------------------------------------------------
class ClipAdamEMA:
    """clip_grad_norm_(params, max_norm) + torch.optim.Adam(params, lr, betas, eps).step() + zero_grad() + the EMA update of
    ema_params (a parallel list, for example the parameters of a deep copy that samples), in three launches per step().

    step() returns the device record (total_norm, coef, nonfinite flag, 0) without reading it: no .item(), no synchronisation, and
    no allocation after the first call.  The gradients are taken from p.grad at every call; a parameter whose .grad is None is left
    alone with its state, its own step count and its EMA entry (a deep copy already equals it), as torch.optim.Adam leaves it.
    The per-tensor pointer table goes to the device from pinned memory on the current stream, whenever it differs from the one
    already there (the gradients usually keep their addresses from step to step).  zero_grad is folded into step() by
    default (g = 0 is written by the update; the .grad tensors stay allocated).  max_norm=None: no clipping (coef = 1).
    skip_nonfinite: a step whose total norm is inf or NaN writes nothing at all -- the gradients included, so they keep their
    values: call zero_grad() when the returned flag is up.

    state_dict() / load_state_dict() use torch.optim.Adam's layout (the reference's `opt0` checkpoint entry), plus the EMA counter
    under "ema_step" / "ema_copied"."""

    _update_entry = "fd_opt_adam_ema_f32"        # the third launch of step(): the update rule (ClipRAdamEMA has RAdam's)

    def __init__(self, params, ema_params=None, lr=1e-4, betas=(0.9, 0.99), eps=1e-8, max_norm=1.0, ema_beta=0.995,
                 ema_update_every=10, ema_update_after_step=100, ema_inv_gamma=1.0, ema_power=2 / 3, ema_min_value=0.0,
                 skip_nonfinite=False):
        fn = type(self).__name__
        if isinstance(params, torch.Tensor):
            raise RuntimeError(f"{fn}: params must be an iterable of tensors (got one tensor)")
        params = list(params)
        ema = None if ema_params is None else list(ema_params)
        if not params:
            raise RuntimeError(f"{fn}: params is empty")
        _check_f32(fn, [(f"params[{i}]", p) for i, p in enumerate(params)])
        if ema is not None:
            _check_f32(fn, [(f"ema_params[{i}]", e) for i, e in enumerate(ema)])
        ok = isinstance(lr, (int, float)) and lr >= 0 and len(betas) == 2 and all(0 <= b < 1 for b in betas) and eps >= 0 and \
            (max_norm is None or max_norm >= 0) and 0 <= ema_beta <= 1 and ema_update_every >= 1
        if not ok:
            raise RuntimeError(f"{fn}: invalid hyperparameters lr={lr} betas={betas} eps={eps} max_norm={max_norm} ema_beta={ema_beta} "
                               f"ema_update_every={ema_update_every}")
        if ema is not None and (len(ema) != len(params) or any(e.shape != p.shape for e, p in zip(ema, params))):
            raise RuntimeError(f"{fn}: inconsistent shapes: ema_params must be a parallel list of tensors shaped as params")
        for name, lst in (("params", params), ("ema_params", ema or [])):
            for i, p in enumerate(lst):
                if p.numel() < 1 or not p.is_contiguous():
                    raise RuntimeError(f"{fn}: unsupported shape {name}[{i}]{tuple(p.shape)} strides {p.stride()} (dense, not empty)")
        _check_gpu(fn, [(f"params[{i}]", p) for i, p in enumerate(params)] + [(f"ema_params[{i}]", e) for i, e in enumerate(ema or [])])
        self.params, self.ema_params = params, ema
        self.lr, self.betas, self.eps, self.max_norm, self.skip_nonfinite = float(lr), tuple(map(float, betas)), float(eps), max_norm, \
            bool(skip_nonfinite)
        self.ema_args = dict(beta=ema_beta, update_every=ema_update_every, update_after_step=ema_update_after_step,
                             inv_gamma=ema_inv_gamma, power=ema_power, min_value=ema_min_value)
        self.ema_step, self.ema_copied = 0, False
        dev = self.device = params[0].device
        nt = self.nt = len(params)
        chunks = chunk_table([p.numel() for p in params])
        self.nchunk = len(chunks)
        with torch.cuda.device(dev):
            if L.lib().fd_opt_chunk_elems() != CHUNK:
                raise RuntimeError(f"{fn}: the library cuts chunks of {L.lib().fd_opt_chunk_elems()} elements, this module of {CHUNK}")
            self._chunks = torch.from_numpy(chunks).to(dev)
            offs = np.cumsum([0] + [(p.numel() + 3) & ~3 for p in params])           # every state tensor starts 16-byte aligned
            self._m, self._v = torch.zeros(int(offs[-1]), device=dev), torch.zeros(int(offs[-1]), device=dev)
            self.exp_avg = [self._m[o:o + p.numel()].view(p.shape) for o, p in zip(offs, params)]
            self.exp_avg_sq = [self._v[o:o + p.numel()].view(p.shape) for o, p in zip(offs, params)]
            self._steps = torch.zeros(nt, device=dev, dtype=torch.int32)
            self._part, self._rec = torch.empty(self.nchunk, device=dev), torch.zeros(4, device=dev)
            self._table = torch.zeros(nt, 8, device=dev, dtype=torch.int64)
            self._pinned = torch.zeros(nt, 8, dtype=torch.int64).pin_memory()
            self._uploaded, self._event = None, torch.cuda.Event()
        self._host = np.zeros((nt, 8), dtype=np.int64)
        self._host[:, 2] = [m.data_ptr() for m in self.exp_avg]
        self._host[:, 3] = [v.data_ptr() for v in self.exp_avg_sq]

    def _upload_table(self):
        fn, h = type(self).__name__ + ".step", self._host
        grads = [p.grad for p in self.params]
        for i, (p, g) in enumerate(zip(self.params, grads)):
            if g is None:
                continue
            if g.dtype != torch.float32:
                raise RuntimeError(f"{fn}: the gradient of params[{i}] must be float32 (got {g.dtype})")
            if g.shape != p.shape or not g.is_contiguous():
                raise RuntimeError(f"{fn}: inconsistent shapes: the gradient of params[{i}]{tuple(p.shape)} is {tuple(g.shape)} with "
                                   f"strides {g.stride()} (dense, shaped as the parameter)")
            if g.device != self.device:
                raise RuntimeError(f"{fn}: the gradient of params[{i}] lives on {g.device}, the parameters on {self.device}")
        h[:, 0] = [p.data_ptr() for p in self.params]
        h[:, 1] = [0 if g is None else g.data_ptr() for g in grads]
        h[:, 4] = 0 if self.ema_params is None else [e.data_ptr() for e in self.ema_params]
        aligned = ((h[:, 0] | h[:, 1] | h[:, 4]) & 15) == 0
        h[:, 5] = np.where(h[:, 1] != 0, 1 + 2 * aligned, 0)
        if self._uploaded is None or not np.array_equal(h, self._uploaded):
            if self._uploaded is not None:
                self._event.synchronize()                # the pinned buffer's last copy has left it (a changed table is rare)
            self._pinned.numpy()[:] = h
            self._table.copy_(self._pinned, non_blocking=True)
            self._event.record()
            self._uploaded = h.copy()

    def step(self, zero_grad=True, ema_mode=None, ema_decay=None):
        """One update on the current stream.  ema_mode / ema_decay override the schedule for this call (0: leave the EMA alone, 1: copy,
        2: decayed update).  Returns the device record (4 floats): total_norm, coef, nonfinite, 0."""
        if ema_mode is not None and (ema_mode not in (0, 1, 2) or (ema_mode == 2 and ema_decay is None)):
            raise RuntimeError(f"{type(self).__name__}.step: ema_mode must be 0, 1 or 2, with an ema_decay for 2 (got {ema_mode}, "
                               f"{ema_decay})")
        with torch.cuda.device(self.device):
            self._upload_table()
            s0 = self.ema_step
            self.ema_step += 1
            if self.ema_params is None:
                mode, decay = 0, 0.0
            elif ema_mode is not None:
                mode, decay = ema_mode, float(ema_decay or 0.0)
            else:
                mode, decay = ema_schedule(s0, self.ema_copied, **self.ema_args)
            self.ema_copied = self.ema_copied or mode != 0
            st, skip = stream(self.device), int(self.skip_nonfinite)
            L.call("fd_opt_sumsq_f32", ptr(self._chunks), ptr(self._table), ptr(self._part), self.nchunk, st)
            L.call("fd_opt_clip_coef", ptr(self._part), self.nchunk, ptr(self._table), ptr(self._steps), self.nt,
                   -1.0 if self.max_norm is None else float(self.max_norm), skip, ptr(self._rec), st)
            L.call(self._update_entry, ptr(self._chunks), ptr(self._table), ptr(self._steps), ptr(self._rec), self.nchunk, self.lr,
                   self.betas[0], self.betas[1], self.eps, mode, decay, int(bool(zero_grad)), skip, st)
        return self._rec

    def zero_grad(self):
        """the gradients to zero, kept allocated (step() does this itself unless called with zero_grad=False)"""
        grads = [p.grad for p in self.params if p.grad is not None]
        if grads:
            torch._foreach_zero_(grads)

    def steps(self):
        """the Adam step count of every parameter (reads the device)"""
        return self._steps.cpu().tolist()

    def _group(self):
        g = torch.optim.Adam([torch.zeros(1)], lr=self.lr, betas=self.betas, eps=self.eps).state_dict()["param_groups"][0]
        return g

    def state_dict(self):
        sd = adam_state_pack(self.steps(), [m.clone() for m in self.exp_avg], [v.clone() for v in self.exp_avg_sq], self._group())
        sd["ema_step"], sd["ema_copied"] = self.ema_step, self.ema_copied
        return sd

    def load_state_dict(self, sd):
        steps, m, v = adam_state_unpack(sd, self.nt)
        for i, p in enumerate(self.params):
            for name, t in (("exp_avg", m[i]), ("exp_avg_sq", v[i])):
                if t is not None and (not isinstance(t, torch.Tensor) or t.shape != p.shape):
                    raise RuntimeError(f"{type(self).__name__}.load_state_dict: inconsistent shapes: {name} of parameter {i} is "
                                       f"{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}, the parameter "
                                       f"{tuple(p.shape)}")
        with torch.no_grad():
            for i in range(self.nt):
                for dst, src in ((self.exp_avg[i], m[i]), (self.exp_avg_sq[i], v[i])):
                    if src is None:
                        dst.zero_()
                    else:
                        dst.copy_(src)
            self._steps.copy_(torch.tensor(steps, dtype=torch.int32))
        group = sd["param_groups"][0]
        self.lr, self.betas, self.eps = float(group.get("lr", self.lr)), tuple(map(float, group.get("betas", self.betas))), \
            float(group.get("eps", self.eps))
        self.ema_step, self.ema_copied = int(sd.get("ema_step", self.ema_step)), bool(sd.get("ema_copied", self.ema_copied))


class ClipRAdamEMA(ClipAdamEMA):
    """ClipAdamEMA with torch.optim.RAdam(params, lr, betas, eps, weight_decay=0)'s update in Adam's place (fd_opt_radam_ema_f32;
    radam_scalars has the rule): what the reference optimises two U-Nets with (src/DADiff.py:1598-1602), after one
    clip_grad_norm_ over both and before one EMA of the whole model.  One object over list(unet0.parameters()) +
    list(unet1.parameters()) is therefore the reference's joint clip, its two optimisers and its EMA, in the same three launches
    per step(): every tensor has its own step count and its own branch of the rule.  The constructor's arguments are
    ClipAdamEMA's; betas default to RAdam's (0.9, 0.999), which is what the reference runs with -- not its adam_betas.  There is
    no weight decay.  state_dict() / load_state_dict() use torch.optim.RAdam's layout."""

    _update_entry = "fd_opt_radam_ema_f32"

    def __init__(self, params, ema_params=None, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, max_norm=1.0, ema_beta=0.995,
                 ema_update_every=10, ema_update_after_step=100, ema_inv_gamma=1.0, ema_power=2 / 3, ema_min_value=0.0,
                 skip_nonfinite=False):
        super().__init__(params, ema_params, lr, betas, eps, max_norm, ema_beta, ema_update_every, ema_update_after_step,
                         ema_inv_gamma, ema_power, ema_min_value, skip_nonfinite)

    def _group(self):
        return torch.optim.RAdam([torch.zeros(1)], lr=self.lr, betas=self.betas, eps=self.eps,
                                 weight_decay=0.0).state_dict()["param_groups"][0]

    def load_state_dict(self, sd):
        fn = "ClipRAdamEMA.load_state_dict"
        for g in sd["param_groups"]:
            if optimizer_kind(g) == "adam":
                raise RuntimeError(f"{fn}: the state was written by torch.optim.Adam (ClipAdamEMA), this is torch.optim.RAdam "
                                   f"(ClipRAdamEMA): Adam and RAdam state do not load into each other")
            if g.get("weight_decay", 0) != 0:
                raise RuntimeError(f"{fn}: weight_decay={g['weight_decay']} is not supported (the reference runs RAdam with 0)")
        super().load_state_dict(sd)


# ---- data-parallel training: the ordered gradient sum --------------------------------------------------------------------------------
def ordered_sum(rounds):
    """The sum GradReducer computes, in numpy: `rounds` is a sequence of (W, N) float32 arrays, one per call, row r from rank r.
    acc = 0; then acc = acc + rounds[a][r] for a outer and r inner, every add rounded to float32: global micro-batch a W + r in
    its own order, which is the order a single process accumulates its A W micro-batches in."""
    acc = None
    for rows in rounds:
        rows = np.asarray(rows, dtype=np.float32)
        if rows.ndim != 2 or (acc is not None and rows.shape[1:] != acc.shape):
            raise RuntimeError(f"ordered_sum: every round is a (W, N) array with one N (got {rows.shape})")
        if acc is None:
            acc = np.zeros(rows.shape[1], dtype=np.float32)
        for r in range(rows.shape[0]):
            acc = (acc + rows[r]).astype(np.float32)
    if acc is None:
        raise RuntimeError("ordered_sum: no rounds")
    return acc


def dp_micro(a, world, rank):
    """the global number of micro-batch `a` of rank `rank` among `world`: a world + rank.  With A micro-batches per rank the step
    has A world of them, and the ranks' numbers of round a are consecutive: the rank-ordered sum of round after round adds them
    in global order."""
    if world < 1 or not 0 <= rank < world or a < 0:
        raise RuntimeError(f"dp_micro: invalid arguments a={a} world={world} rank={rank}")
    return int(a) * int(world) + int(rank)


class GradReducer:
    """The gradient sum of data-parallel training over ClipAdamEMA's tables: GradReducer(opt, group=None), W = the size of the
    (initialised) process group, None being the default one.  Every rank calls reduce() once per micro-batch, after all of that
    micro-batch's backward passes (the U-Nets' parameter sets are disjoint: each tensor holds one contribution):

      1. fd_grads_pack_f32: the gradients of the tensors that have one go to a flat buffer (the layout of the optimiser's moments:
         offs = cumsum((numel + 3) & ~3), padding zero), the micro-batch's losses into the tail behind them, and the gradients are
         zeroed, so the next backward starts from 0 as a single process's does after zero_grad;
      2. parallel.all_gather_flat: every rank receives every rank's buffer, (W, N);
      3. fd_grads_rank_sum_f32: v = first ? 0 : acc; v = v + recv[r] for r = 0 .. W - 1 in that order; on the last micro-batch v
         goes to the .grad tensors, otherwise to acc.

    With micro-batch a of rank r being global micro-batch a W + r (dp_micro), the .grad tensors after the last call hold, bit for
    bit, what a single process accumulates over the A W micro-batches in its own order, on every rank; opt.step() then runs
    unchanged, and replicated optimisers and EMAs stay identical without a broadcast.  losses() gives the summed losses, one 0-dim
    tensor per U-Net, in the same order of addition.  Memory: (W + 2) N floats, N = the padded parameter count + 4.  A tensor
    whose .grad is None on this rank contributes zeros and is not written.  There is no CPU path."""

    def __init__(self, opt, group=None):
        import torch.distributed as dist
        fn = "GradReducer"
        if not isinstance(opt, ClipAdamEMA):
            raise RuntimeError(f"{fn}: opt must be a ClipAdamEMA (got {type(opt).__name__})")
        if not (dist.is_available() and dist.is_initialized()):
            raise RuntimeError(f"{fn}: torch.distributed is not initialised (call init_process_group first)")
        self.opt, self.group = opt, group
        self.world, self.rank = dist.get_world_size(group), dist.get_rank(group)
        if not 1 <= self.world <= 64:
            raise RuntimeError(f"{fn}: the group has {self.world} ranks (fd_grads_rank_sum_f32 sums at most 64)")
        dev = self.device = opt.device
        offs = np.cumsum([0] + [(p.numel() + 3) & ~3 for p in opt.params]).astype(np.int64)
        with torch.cuda.device(dev):
            self.tail = int(L.lib().fd_grads_tail_floats())
            self.P, self.N = int(offs[-1]), int(offs[-1]) + self.tail
            self._offs = torch.from_numpy(offs[:-1].copy()).to(dev)
            self.flat, self.acc = torch.zeros(self.N, device=dev), torch.zeros(self.N, device=dev)
            self.recv = torch.zeros(self.world, self.N, device=dev)
        self.n_losses = 0

    def pack(self, losses=(), zero=True):
        """step 1 alone: this rank's gradients and `losses` (at most 4 scalars on the device) into self.flat"""
        opt, dev = self.opt, self.device
        losses = list(losses)
        if len(losses) > self.tail:
            raise RuntimeError(f"GradReducer: the tail holds {self.tail} losses (got {len(losses)})")
        with torch.no_grad(), torch.cuda.device(dev):
            opt._upload_table()
            tail = torch.stack([v.detach().reshape(()).float() for v in losses]) if losses else None
            if tail is not None and tail.device != dev:
                raise RuntimeError(f"GradReducer: the losses live on {tail.device}, the parameters on {dev}")
            L.call("fd_grads_pack_f32", ptr(opt._chunks), ptr(opt._table), ptr(self._offs), opt.nchunk, ptr(self.flat), self.P,
                   ptr(tail), len(losses), int(bool(zero)), stream(dev))
        self.n_losses = len(losses)
        return self.flat

    def rank_sum(self, first, last):
        """step 3 alone: self.recv's rows in rank order onto self.acc (first: onto 0), into the gradients when `last`"""
        opt, dev = self.opt, self.device
        with torch.no_grad(), torch.cuda.device(dev):
            L.call("fd_grads_rank_sum_f32", ptr(opt._chunks), ptr(opt._table), ptr(self._offs), opt.nchunk, ptr(self.recv), self.world,
                   self.N, ptr(self.acc), self.P, int(bool(first)), int(bool(last)), stream(dev))

    def reduce(self, losses=(), first=True, last=True):
        """one micro-batch: pack and zero, all-gather, rank-sum"""
        from .parallel import all_gather_flat
        self.pack(losses, zero=True)
        all_gather_flat(self.flat, self.recv, self.group)
        self.rank_sum(first, last)

    def losses(self):
        """the losses summed so far, one 0-dim device tensor per loss of the last call"""
        return [self.acc[self.P + u].clone() for u in range(self.n_losses)]


# ---- the loop body -----------------------------------------------------------------------------------------------------------------
def train_step(diffusion_or_fn, opt, batch, t=None, noise=None, slice_seeds=None, step=0, schedule=None, objective="pred_res",
               loss_type="l1", normalize=True, reducer=None, ssim_weight=0.0):
    """The loop body of Trainer.train (src/DADiff.py:1689-1725) for one accumulation group: p_losses -> backward per loss ->
    opt.step() (clip, Adam, zero_grad, EMA).  diffusion_or_fn: an object with the reference's ResidualDiffusion attributes, or a
    free model_fn(x_in, [time0, time1]) -> list of (B, 1, H, W) together with schedule, objective and loss_type.  batch:
    [x_start, x_input] in [0, 1] (normalize=True, as ResidualDiffusion.forward takes them), or a list of such pairs: the
    micro-batches of gradient_accumulate_every, each loss scaled by one over their number.  A micro-batch may also be a StoreBatch
    (one, or a list of them), whose t and slice_seeds may stay on the host.  t, noise and slice_seeds belong to the
    micro-batch (lists of them for several); t defaults to torch.randint(0, T, (B,)) as the reference draws it.  `step` keys the
    noise together with slice_seeds.  Returns the losses, one device tensor per U-Net, summed over the micro-batches.
    reducer (a GradReducer over opt; None: a single process, the path above): data-parallel training.  `batch` then holds this
    rank's micro-batches of the step, the a-th of them being global micro-batch a W + rank of len(batch) W (dp_micro: the caller
    draws its indices, t and seeds under that number); each loss is scaled by one over len(batch) W, and reducer.reduce() follows
    every micro-batch's backward passes.  The gradients opt.step() sees and the losses returned are then, on every rank, bit for
    bit those of a single process over all len(batch) W micro-batches.
    ssim_weight: p_losses_fn's, for a free model_fn; a diffusion object brings its own attribute (0.0 where it has none)."""
    fn = "train_step"
    if not isinstance(opt, ClipAdamEMA):
        raise RuntimeError(f"{fn}: opt must be a ClipAdamEMA (got {type(opt).__name__})")
    if reducer is not None and (not isinstance(reducer, GradReducer) or reducer.opt is not opt):
        raise RuntimeError(f"{fn}: reducer must be a GradReducer over opt (got {type(reducer).__name__})")
    single = isinstance(batch, StoreBatch)
    if single:
        batch = [batch]
    if not isinstance(batch, (list, tuple)) or not batch:
        raise RuntimeError(f"{fn}: batch must be [x_start, x_input] or a list of such pairs (got {type(batch).__name__})")
    many = not single and isinstance(batch[0], (list, tuple, StoreBatch))
    groups = list(batch) if many or single else [batch]
    if hasattr(diffusion_or_fn, "alphas_cumsum") and hasattr(diffusion_or_fn, "objective"):
        model_fn, schedule, objective, loss_type, ssim_weight = _diffusion_args(fn, diffusion_or_fn)
    elif callable(diffusion_or_fn):
        model_fn = diffusion_or_fn
    else:
        raise RuntimeError(f"{fn}: diffusion_or_fn must be a ResidualDiffusion or a callable (got {type(diffusion_or_fn).__name__})")
    ac, _ = _schedule_tables(fn, schedule)

    def pick(v, i):
        if not many:
            return v
        if v is not None and (not isinstance(v, (list, tuple)) or len(v) != len(groups)):
            raise RuntimeError(f"{fn}: with {len(groups)} micro-batches t, noise and slice_seeds are lists of {len(groups)}")
        return None if v is None else v[i]

    total = None
    n_micro = len(groups) * (1 if reducer is None else reducer.world)
    for i, imgs in enumerate(groups):
        ti = pick(t, i)
        if ti is None and isinstance(imgs, StoreBatch):
            ti = torch.randint(0, ac.numel(), (len(imgs),), device=imgs.device).long()
        if ti is None:
            if not (isinstance(imgs, (list, tuple)) and len(imgs) == 2 and isinstance(imgs[0], torch.Tensor) and imgs[0].is_cuda):
                raise RuntimeError(f"{fn}: a micro-batch must be [x_start, x_input] on the GPU (there is no CPU path)")
            ti = torch.randint(0, ac.numel(), (imgs[0].shape[0],), device=imgs[0].device).long()
        losses = p_losses_fn(model_fn, imgs, ti, schedule, objective, loss_type, pick(noise, i), pick(slice_seeds, i), step,
                             1.0 / n_micro, normalize, ssim_weight=ssim_weight)
        for loss in losses:
            loss.backward()
        det = [loss.detach() for loss in losses]
        if reducer is not None:
            reducer.reduce(det, first=i == 0, last=i == len(groups) - 1)
            continue
        total = det if total is None else [a + b for a, b in zip(total, det)]
    opt.step()
    return total if reducer is None else reducer.losses()
