"""Characterization of ResidualDiffusion._sample's routing, on the CPU: which sampler a call reaches (the group split, the
concurrent sub-batches, ddim_sample, p_sample_loop), with which shapes and which arguments left None, and every draw of x_T and
of the per-slice seeds on the way -- torch.randint, torch.randn, the keyed stream -- in order.  The samplers and the generators are
recording stubs; every tensor a stub hands out carries the number of the draw that made it (slice b of draw n holds 1000 n + b), so a
row also says WHICH draw, and which slices of it, an argument came from.  tests/test_sample_routing_cpu.py compares the rows with
tests/golden/sample_routing.json.  The golden pins behaviour, not correctness: it was recorded before the noise / seed rule of
_sample was gathered into one helper, and a change that is meant to alter the routing regenerates it with

    python tests/sample_routing.py --write
"""
import itertools
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from founddiff_amd import DADiff                                       # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "sample_routing.json")
HW = 8
GIVEN_NOISE, GIVEN_SEEDS = 900, 800                                    # the "draw numbers" of what the caller passes in
AXES = dict(S=(10, 1000), B=(2, 8, 12, 40), streams=(1, 2), msb=(4, 16), noise=(1, 0), seeds=(1, 0), step_noise=(1, 0), last=(1, 0))
CASES = [dict(zip(AXES, v)) for v in itertools.product(*AXES.values())]


def case_id(c):
    return " ".join(f"{k}={v}" for k, v in c.items())


def _tagged(n, shape, dtype):
    """slice b of the tensor holds 1000 n + b"""
    t = torch.arange(shape[0], dtype=dtype) + 1000 * n
    return t.reshape((-1,) + (1,) * (len(shape) - 1)).expand(tuple(shape)).contiguous()


def _desc(t):
    """None, or [shape, tag of the first slice, tag of the last slice]"""
    if t is None:
        return None
    t = torch.as_tensor(t)
    flat = t.reshape(t.shape[0], -1)
    return [list(t.shape), int(flat[0, 0]), int(flat[-1, 0])]


class Recorder:
    """One ResidualDiffusion per sampling_timesteps over one small U-Net; run(case) -> the rows of one _sample call."""

    def __init__(self):
        net = DADiff.UnetRes(dim=32, dim_mults=(1, 2), num_unet=1, condition=True, objective="pred_res", test_res_or_noise="res",
                             clip_cfg=dict(layers=(2, 1, 1, 1), width=16, embed_dim=1024))
        self.difs = {S: DADiff.ResidualDiffusion(net, image_size=HW, timesteps=1000, sampling_timesteps=S, objective="pred_res",
                                                 loss_type="l2", condition=True, sum_scale=0.01) for S in AXES["S"]}
        for dif in self.difs.values():
            dif.ddim_sample = self._ddim_sample
            dif.p_sample_loop = self._p_sample_loop
            dif._sample_concurrent = self._sample_concurrent
            dif._keyed_noise = self._keyed_noise
        self.rows, self.draws = [], 0

    def _draw(self, shape, dtype):
        self.draws += 1
        return _tagged(self.draws, shape, dtype)

    # ---- the stubs
    def _randint(self, low, high, size, **kw):
        self.rows.append(["randint", [low, high], list(size), sorted(kw)])
        return self._draw(size, kw["dtype"])

    def _randn(self, *size, **kw):
        size = size[0] if len(size) == 1 and not isinstance(size[0], int) else size
        self.rows.append(["randn", list(size), sorted(kw)])
        return self._draw(size, torch.float32)

    def _keyed_noise(self, seeds, t, shape):
        self.rows.append(["_keyed_noise", _desc(seeds), int(t), list(shape)])
        return self._draw(shape, torch.float32)

    def _out(self, shape):
        return [torch.zeros(tuple(shape)), torch.zeros(tuple(shape))]

    def _ddim_sample(self, x_input, shape, last=True, noise=None):
        self.rows.append(["ddim_sample", [list(x.shape) for x in x_input], list(shape), bool(last), _desc(noise)])
        return self._out(shape)

    def _p_sample_loop(self, x_input, shape, last=True, noise=None, step_noise=None, slice_seeds=None):
        self.rows.append(["p_sample_loop", [list(x.shape) for x in x_input], list(shape), bool(last), _desc(noise),
                          step_noise is not None, _desc(slice_seeds)])
        return self._out(shape)

    def _sample_concurrent(self, x_in, size, noise, nsl, seeds=None):
        self.rows.append(["_sample_concurrent", list(x_in.shape), list(size), _desc(noise), int(nsl), _desc(seeds)])
        return self._out(size)

    def run(self, c):
        dif = self.difs[c["S"]]
        dif.streams, dif.max_sub_batch = c["streams"], c["msb"]
        shape = (c["B"], 1, HW, HW)
        self.rows, self.draws = [], 0
        saved = DADiff._affine, torch.randint, torch.randn
        DADiff._affine = lambda x, a, b: x * a + b
        torch.randint, torch.randn = self._randint, self._randn
        try:
            out = dif._sample([torch.full(shape, 0.5)], c["B"], bool(c["last"]),
                              _tagged(GIVEN_NOISE, shape, torch.float32) if c["noise"] else None,
                              (lambda t: None) if c["step_noise"] else None,
                              _tagged(GIVEN_SEEDS, (c["B"],), torch.int64) if c["seeds"] else None)
        finally:
            DADiff._affine, torch.randint, torch.randn = saved
        self.rows.append(["returns", [list(o.shape) for o in out]])
        return self.rows


def snapshot():
    rec = Recorder()
    return {case_id(c): rec.run(c) for c in CASES}


def write(path=GOLDEN):
    g = snapshot()
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(f' {json.dumps(k)}: {json.dumps(v, separators=(",", ":"))}' for k, v in g.items()) + "\n}\n")
    return g


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python tests/sample_routing.py --write")
    g = write()
    print(f"{GOLDEN}: {len(g)} cases, {len({json.dumps(v) for v in g.values()})} distinct, {os.path.getsize(GOLDEN)} bytes")
