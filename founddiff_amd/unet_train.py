"""The reference's Unet (src/DADiff.py:530-740) for training: every activation between init_conv and final_conv stays channel-last
(B, H, W, C) on this project's HIP kernels.

    per level down:  Mamba_block -> ResnetBlock -> (skip) -> Downsample | Conv2d 3x3     mamba_block_train, resblock_train,
    middle:          ResnetBlock -> Mamba_block                                          resample_train
    per level up:    cat(skip) -> ResnetBlock -> Mamba_block -> Upsample | Conv2d 3x3
    end:             cat(init) -> ResnetBlock -> final_conv

torch.cat runs on the last axis and there is no layout copy.  The frozen dose_encoder, the time / prompt MLPs and the two outer
convolutions (init_conv 7x7 on 2 planes, final_conv 1x1 to 1 plane: weight gradients of 6 K and 64 elements) stay with torch, the
latter two on channels-last memory -- unless unet_trunk_forward is given init_fn / final_fn (outer_conv_train), as the project's
own model does (DADiff.Unet.train_forward): then the whole step's activation work is on HIP kernels and deterministic.

Binding for a training run:

    import DADiff, founddiff_amd.unet_train as ut
    DADiff.Unet.forward = ut.unet_forward

`UnetTrunk(dim, dim_mults, ...)` is the same network without the encoders, forward(x, time, dose_embedding, c), with the
reference's parameter names, shapes, d_states and initialisation, for code that does not import the reference.
"""
import math

import torch

from .mamba_block_train import MambaBlock, mamba_block_forward
from .resample_train import resample_nhwc
from .resblock_train import ResnetBlock, resnet_block_nhwc

__all__ = ["unet_forward", "unet_trunk_forward", "UnetTrunk"]


def _nhwc(x):
    """NCHW -> (B, H, W, C), dense: a view when x lives in channels-last memory, as torch's convolutions leave it"""
    return x.permute(0, 2, 3, 1).contiguous()


def unet_trunk_forward(self, x, time, dose_embedding, c, init_fn=None, final_fn=None):
    """Unet.forward after the dose encoder (src/DADiff.py:700-740) on the reference's attribute names: x (B, input_channels, H, W),
    time (B,), dose_embedding (B, context_dim), c (B, 1, 256) -> (B, out_dim, H, W).  H and W must be multiples of
    2 ** (levels - 1), as in the reference (whose torch.cat fails otherwise).  init_fn(x, weight, bias) -> (B, H, W, dim) and
    final_fn(x (B, H, W, dim), weight, bias) -> (B, 1, H, W) replace torch's two outer convolutions
    (outer_conv_train.init_conv_fn / final_conv_fn); None: torch on channels-last memory."""
    named = (("x", x), ("time", time), ("dose_embedding", dose_embedding), ("c", c))
    for name, v in named:
        if not isinstance(v, torch.Tensor):
            raise RuntimeError(f"unet_forward: {name} must be a tensor (got {type(v).__name__})")
    for name, v in named:
        if not v.is_cuda:
            raise RuntimeError(f"unet_forward: {name} must live on the GPU (there is no CPU path)")
    if x.dim() != 4 or x.shape[1] != self.init_conv.in_channels:
        raise RuntimeError(f"unet_forward: inconsistent shapes x{tuple(x.shape)} (expected (B, {self.init_conv.in_channels}, H, W))")
    levels = len(self.downs)
    if x.shape[2] % (1 << (levels - 1)) or x.shape[3] % (1 << (levels - 1)):
        raise RuntimeError(f"unet_forward: unsupported shape H={x.shape[2]} W={x.shape[3]} (multiples of {1 << (levels - 1)}: every "
                           "Downsample needs an even size)")
    if init_fn is None:
        x = _nhwc(self.init_conv(x.contiguous(memory_format=torch.channels_last)))
    else:
        x = init_fn(x.contiguous(), self.init_conv.weight, self.init_conv.bias)
    r = x
    t = self.time_mlp(time)
    prompt_embedding = torch.softmax(self.text_mlp(dose_embedding), dim=1) * self.prompt
    t = t + self.prompt_mlp(prompt_embedding)

    def mamba(block, x):
        return mamba_block_forward(block, x.permute(0, 3, 1, 2), c, t).permute(0, 2, 3, 1)

    h = []
    for res_block, attn, downsample in self.downs:
        x = mamba(attn, x)
        x = resnet_block_nhwc(res_block, x)
        h.append(x)
        x = resample_nhwc(downsample, x)
    x = resnet_block_nhwc(self.mid_block, x)
    x = mamba(self.mid_attn, x)
    for res_block, attn, upsample in self.ups:
        x = torch.cat((x, h.pop()), dim=3)
        x = resnet_block_nhwc(res_block, x)
        x = mamba(attn, x)
        x = resample_nhwc(upsample, x)
    x = torch.cat((x, r), dim=3)
    x = resnet_block_nhwc(self.final_res_block, x)
    if final_fn is None:
        return self.final_conv(x.permute(0, 3, 1, 2))
    return final_fn(x, self.final_conv.weight, self.final_conv.bias)


def unet_forward(self, x, time, x_self_cond=None):
    """Unet.forward (src/DADiff.py:685-740): x (B, 2, H, W) = cat(x_t, x_input), time (B,) -> (B, 1, H, W).  Reads the
    reference's attribute names; the dose_encoder sees plane 1 of x three times, as in the reference.  Raises RuntimeError, before
    the trunk launches anything, for CPU tensors, a size that is no multiple of 2 ** (levels - 1), cross=True blocks and whatever
    mamba_block_forward, resnet_block_nhwc and resample_nhwc do not support."""
    if getattr(self, "self_condition", False):
        x_self_cond = torch.zeros_like(x) if x_self_cond is None else x_self_cond
        x = torch.cat((x_self_cond, x), dim=1)
    _, dose_embedding, context_embedding = self.dose_encoder(x[:, 1, :, :].unsqueeze(1).repeat(1, 3, 1, 1))
    return unet_trunk_forward(self, x, time, dose_embedding, context_embedding.unsqueeze(1))


class _SinusoidalPosEmb(torch.nn.Module):
    """src/DADiff.py:173-185"""

    def __init__(self, dim):
        super().__init__()
        self.dim = dim

    def forward(self, x):
        half = self.dim // 2
        emb = torch.exp(torch.arange(half, device=x.device) * -(math.log(10000) / (half - 1)))
        emb = x[:, None] * emb[None, :]
        return torch.cat((emb.sin(), emb.cos()), dim=-1)


def _d_state(level):
    return 4 if level == 0 else int(4 * 2 ** level)


class UnetTrunk(torch.nn.Module):
    """The reference's Unet without its encoders: init_conv, time_mlp, prompt, text_mlp, prompt_mlp, downs.i.{0,1,2} =
    (ResnetBlock, Mamba_block, Downsample | Conv2d 3x3), mid_block, mid_attn, ups.i.{0,1,2} = (ResnetBlock, Mamba_block, Upsample |
    Conv2d 3x3), final_res_block, final_conv.  Parameter names, shapes and initialisation are the reference's, and so are the
    d_states: 4 * 2 ** level on the way down, 32 in the middle, 4 * 2 ** (3 - i) for ups.i whatever the depth (src/DADiff.py:663-666).
    The trunk keys of arch.da_unet_spec(dim, dim_mults) load with strict=True.  forward(x, time, dose_embedding, c): x
    (B, input_channels, H, W), time (B,), dose_embedding (B, context_dim) and c (B, 1, 256) as the dose encoder gives them."""

    def __init__(self, dim, dim_mults=(1, 2, 4, 8), channels=1, input_channels=2, context_dim=1024, resnet_block_groups=8):
        super().__init__()
        nn = torch.nn
        self.channels = channels
        self.init_conv = nn.Conv2d(input_channels, dim, 7, padding=3)
        dims = [dim] + [dim * m for m in dim_mults]
        in_out = list(zip(dims[:-1], dims[1:]))
        time_dim = dim * 4
        self.time_mlp = nn.Sequential(_SinusoidalPosEmb(dim), nn.Linear(dim, time_dim), nn.GELU(), nn.Linear(time_dim, time_dim))
        self.prompt = nn.Parameter(torch.rand(1, time_dim))
        self.text_mlp = nn.Sequential(nn.Linear(context_dim, time_dim), nn.SiLU(), nn.Linear(time_dim, time_dim))
        self.prompt_mlp = nn.Linear(time_dim, time_dim)
        block = lambda i, o: ResnetBlock(i, o, time_emb_dim=time_dim, groups=resnet_block_groups)
        self.downs, self.ups = nn.ModuleList([]), nn.ModuleList([])
        n = len(in_out)
        for ind, (di, do) in enumerate(in_out):
            self.downs.append(nn.ModuleList([
                block(di, di), MambaBlock(di, _d_state(ind), time_dim),
                nn.Conv2d(di, do, 4, 2, 1) if ind < n - 1 else nn.Conv2d(di, do, 3, padding=1)]))
        mid = dims[-1]
        self.mid_block = block(mid, mid)
        self.mid_attn = MambaBlock(mid, _d_state(3), time_dim)
        for ind, (di, do) in enumerate(reversed(in_out)):
            up = nn.Sequential(nn.Upsample(scale_factor=2, mode="nearest"), nn.Conv2d(do, di, 3, padding=1)) if ind < n - 1 else \
                nn.Conv2d(do, di, 3, padding=1)
            self.ups.append(nn.ModuleList([block(do + di, do), MambaBlock(do, _d_state(3 - ind), time_dim), up]))
        self.out_dim = channels
        self.final_res_block = block(dim * 2, dim)
        self.final_conv = nn.Conv2d(dim, self.out_dim, 1)

    forward = unet_trunk_forward
