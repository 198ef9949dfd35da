"""The residual schedule and the strict checkpoint load, in a module of their own: the samplers (DADiff.py) and the Trainer
(trainer.py) both need them and neither needs the other.  `founddiff_amd.DADiff` re-exports both names."""
import torch


def residual_schedule(timesteps=1000, after_init=False):
    """The 12 schedule vectors (src/DADiff.py:946-1027 for __init__, 1033-1118 for init())."""
    import torch.nn.functional as F
    betas = torch.linspace(1e-4, 0.02, timesteps, dtype=torch.float32)
    acp = torch.cumprod(1.0 - betas, dim=0)
    acs = 1 - acp ** 0.5
    b2cs = 1 - acp
    acs_prev = F.pad(acs[:-1], (1, 0), value=1.0)
    b2cs_prev = F.pad(b2cs[:-1], (1, 0), value=1.0)
    alphas = acs - acs_prev
    betas2 = b2cs - b2cs_prev
    alphas[0] = alphas[1] if after_init else 0
    betas2[0] = betas2[1] if after_init else 0
    pv = betas2 * b2cs_prev / b2cs
    pv[0] = 0
    out = dict(alphas=alphas, alphas_cumsum=acs, one_minus_alphas_cumsum=1 - acs, betas2=betas2,
               betas=torch.sqrt(betas2), betas2_cumsum=b2cs, betas_cumsum=torch.sqrt(b2cs),
               posterior_mean_coef1=b2cs_prev / b2cs,
               posterior_mean_coef2=(betas2 * acs_prev - b2cs_prev * alphas) / b2cs,
               posterior_mean_coef3=betas2 / b2cs, posterior_variance=pv,
               posterior_log_variance_clipped=torch.log(pv.clamp(min=1e-20)))
    out["posterior_mean_coef1"][0] = 0
    out["posterior_mean_coef2"][0] = 0
    out["posterior_mean_coef3"][0] = 1
    out["one_minus_alphas_cumsum"][-1] = 1e-6
    return {k: v.to(torch.float32) for k, v in out.items()}


def load_weights(module, state_dict, what="checkpoint"):
    """`load_state_dict` the way the reference's strict `Trainer.load` does (src/DADiff.py:1655-1663) for every
    key that is live on the sampling path: dead weight is dropped by the modules' own `load_state_dict`, the
    12 schedule buffers may be absent (they are re-derived by `init()`), anything else missing or unexpected
    raises -- a checkpoint of another dim / dim_mults / num_unet / input_condition must not leave zero-
    initialised weights behind silently."""
    res = module.load_state_dict(state_dict, strict=False)
    sched = set(residual_schedule(1000).keys())
    missing = [k for k in res.missing_keys if k not in sched]
    unexpected = list(res.unexpected_keys)
    if missing or unexpected:
        raise RuntimeError(f"{what} does not match this model: {len(missing)} live keys missing "
                           f"(e.g. {missing[:3]}), {len(unexpected)} unexpected (e.g. {unexpected[:3]})")
    return res
