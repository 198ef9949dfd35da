"""This project's extensions of the reference's sampling API: ensembles (`sample_ensemble`), a slice as overlapping tiles
(`sample_tiled`), both at once (`sample_ensemble(tile=...)`), and ensembles over the orientations of the square
(`sample_ensemble(orientations=...)`), as a mixin of `DADiff.ResidualDiffusion`.

`DADiff.py` keeps the reference-shaped API (`sample`, `_sample`, the loops; the Trainer is `trainer.py`); everything here is built
on it and adds no loop of the samplers but the per-step fused one.  The host class gives `_sample`, `_range_checked`, `_slice_seeds`,
`_keyed_noise`, `_x_T_into`, `_cond_rows`, `_plan` (an `objectives.SamplePlan`: its `mode` and `two_engines` are read here),
`_plan_unets`, `_engines`, `_group_rows`, `_o01`, the `_obj_*` tables and `_anc_chunks`, and the units of an image as `_normalize` /
`_unnormalize` ([0, 1] <-> [-1, 1]).  Three pieces are shared by every path below:

    TilePlan       the geometry of a tiled call on the device, built and cached whole by `_tile_plan`; every launch takes its
                   geometry arguments from `TilePlan.geometry`
    _tiled_call    the preamble of a tiled call: argument checks, the float slices, the slice seeds, the plan, the row limit
    _rows_final    the final images of R rows through `_sample`, pass by pass: the one loop that calls `_sample`
"""
import ctypes as C
import functools
from collections import namedtuple
from typing import NamedTuple

import numpy as np
import torch

from . import _lib as L
from .engine import _p
from .ensemble import ensemble_passes, ensemble_seeds, orientation_codes, orientation_inverse, quantile_table
from .metrics import ensemble_quantiles, ensemble_stats
from .tiling import tile_pair, tile_passes, tile_plan, tile_seeds, tile_weights, tiled_ensemble_seeds

# sample_ensemble: mean, std (B,1,H,W) in [0, 1] units, spread (B,), samples (B,K,1,H,W) or None
EnsembleResult = namedtuple("EnsembleResult", ["mean", "std", "spread", "samples"])
# sample_ensemble(quantiles=levels): the same four, quantiles (B,Q,1,H,W) in the units of mean, levels the tuple of Q levels
EnsembleQuantiles = namedtuple("EnsembleQuantiles", ["mean", "std", "spread", "samples", "quantiles", "levels"])


def _stream(t):
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _ensemble_result(samples, return_samples):
    """The EnsembleResult of the K final images per slice, samples (B,K,1,H,W)"""
    mean, std, spread = ensemble_stats(samples)
    return EnsembleResult(mean, std, spread, samples if return_samples else None)


class TilePlan(NamedTuple):
    """The plan of tiling.py for H x W slices as my x mx tiles of th x tw pixels, on the device: origins ys (my,), xs (mx,) int32,
    weights wy (my,th), wx (mx,tw) float32, x4 = (xs % 4 == 0).all()"""
    ys: torch.Tensor
    xs: torch.Tensor
    wy: torch.Tensor
    wx: torch.Tensor
    my: int
    mx: int
    x4: int
    th: int
    tw: int
    H: int
    W: int

    @property
    def T(self):
        """tiles per slice"""
        return self.my * self.mx

    def tables(self):
        """the pointer arguments of a launch that blends: weights, then origins"""
        return _p(self.wy), _p(self.wx), _p(self.ys), _p(self.xs)

    def geometry(self, *groups):
        """the geometry arguments of a launch over `groups` row groups of T tiles each: (B,) slices, or (B, K) slices and replicas"""
        return (*groups, self.H, self.W, self.th, self.tw, self.my, self.mx, self.x4)


def _fuse_keyword(fn):
    """sample_tiled's keyword-only `fuse`: "final" (the default) or "step".  It is taken here, in front of the method, and handed to
    it as self._tile_fuse for the length of the call, so that the method keeps the parameter list tests/test_tiling_cpu.py pins
    (inspect.signature follows __wrapped__ to it and therefore does NOT show `fuse`: the docstring is where it is documented)."""
    @functools.wraps(fn)
    def sample_tiled(self, *args, fuse="final", **kw):
        if fuse not in ("final", "step"):
            raise RuntimeError(f"sample_tiled: fuse must be 'final' or 'step' (got {fuse!r})")
        self._tile_fuse = fuse
        try:
            return fn(self, *args, **kw)
        finally:
            self._tile_fuse = "final"
    return sample_tiled


class TiledSampling:
    """sample_ensemble, sample_tiled and their helpers: see the module's docstring for what the host class gives"""

    @torch.no_grad()
    def sample_ensemble(self, x_input, n_samples, slice_seeds=None, return_samples=False, *, tile=None, overlap=0,
                        tile_condition="tile", tile_fuse="final", quantiles=None, orientations=None):
        """K = n_samples keyed realisations of every slice of x_input = [ldct (B,1,H,W) in [0,1]], reduced on the device: an
        EnsembleResult of the per-pixel mean and sample standard deviation over a slice's K final images (both (B,1,H,W), in the
        [0, 1] units of sample()[-1]), spread (B,) = sqrt(mean over pixels of std^2), and the images themselves (B,K,1,H,W) when
        `return_samples`.  Replica k of slice b is the image sample([x[b:b+1]], slice_seeds=[ensemble_seeds(slice_seeds, K)[b, k]])
        returns, bit for bit: x_T -- and the step noise of the ancestral sampler -- is the keyed stream of the replica's seed on
        every path.  The DA-CLIP tower runs once per slice; the B K rows (slice-major) run in passes of at most streams x
        max_sub_batch through the paths of sample(), and nothing returned depends on that cut or on B.
        `tile` (keyword-only, with `overlap`, `tile_condition`, `tile_fuse`; None: all of the above, unchanged): every replica is
        sampled as overlapping tiles.  Replica k of slice b is then, bit for bit, the final image of sample_tiled([x[b:b+1]],
        tile, overlap, slice_seeds=[ensemble_seeds(slice_seeds, K)[b, k]], condition=tile_condition, fuse=tile_fuse), on both
        samplers and for every plan; the result has the same shapes and units.  The rows are tiling.tiled_ensemble_seeds':
        replica first, then tile, row ((b K + k) my + iy) mx + ix, at most 65535 of them.  The tower runs once per slice and tile
        ("tile") or once per slice ("slice"), never per replica: a slice's T conditioning rows and input tiles are repeated for
        its K replicas.  tile_fuse="final": one keyed x_T field per (slice, replica), gathered per tile; the B K T rows run
        through the paths of sample() in tile_passes, and fd_tiles_ensemble_f32 takes their final images straight to mean, std
        and spread (the K blended images are written only for `return_samples`) with the bits of fd_tiles_blend_f32 followed by
        fd_ensemble_stats_f32.  tile_fuse="step": the fused loop of sample_tiled over the B K replicas as pseudo-slices, each
        under its replica seed, then fd_ensemble_stats_f32.  Nothing returned depends on B, max_sub_batch, streams or the passes.
        `quantiles` (keyword-only; None: all of the above, the same launches): a sequence of 1 to 8 levels in [0, 1].  The result
        is then an EnsembleQuantiles, whose `quantiles` (B,Q,1,H,W) holds per pixel the levels of the slice's K final images in the
        caller's order (metrics.ensemble_quantiles: the `linear` rule, fd_ensemble_order_f32 on the K images) and whose `levels` is
        the tuple of levels; mean, std, spread and samples are what the call without `quantiles` returns, bit for bit.  On the
        tile_fuse="final" path the K blended images are written for the order kernel and returned only under `return_samples`.
        `orientations` (keyword-only; None: all of the above, the same launches): the geometric self-ensemble.  "d4" (the 8
        orientations of a square slice), "flips" (the four that keep an H != W shape) or a sequence of flip / rot90 codes in 0..15
        (diffusion_train.train_augment's: bit 0 flips H, bit 1 flips W, bits 2-3 are k); replica k takes
        ensemble.orientation_codes(orientations, K, H == W)[k], the set cycled, so K = 16 with "d4" is every orientation under
        two noise seeds.  Replica k of slice b is then, bit for bit, U(sample([T(x[b:b+1])], batch_size=1,
        slice_seeds=[ensemble_seeds(slice_seeds, K)[b, k]])[-1]), T its orientation and U the inverse: x_T and the step noise are
        the replica seed's keyed stream in the ORIENTED frame.  fd_rows_orient_f32 makes the B K oriented input rows; the tower,
        which is not equivariant, runs on oriented inputs once per slice and distinct orientation, and replicas that share one
        share its row (fd_rows_take_f32); the passes are those above; fd_ensemble_orient_stats_f32 reads every final image back
        through its inverse code, so mean, std, spread, `samples` and `quantiles` are in the slice's own frame with the shapes and
        units above.  The std now also holds where the model is not equivariant.  (0,) is the plain ensemble bit for bit, and
        K = 1 with (c,) is sample() on the oriented slice, turned back.  Nothing returned depends on B, max_sub_batch, streams or
        the passes.  Together with `tile` it is not built and raises."""
        K = int(n_samples)
        if K < 1:
            raise RuntimeError(f"sample_ensemble: n_samples must be at least 1 (got {n_samples})")
        if self.input_condition:
            raise RuntimeError("sample_ensemble: input_condition=True is not built (one input plane per slice)")
        if orientations is not None and tile is not None:
            raise RuntimeError("sample_ensemble: orientation ensembles of tiled samples are not built")
        if quantiles is not None:                                        # the levels are checked before any work
            quantiles = tuple(float(q) for q in quantiles)
            quantile_table(quantiles, K)
            ens = self.sample_ensemble(x_input, K, slice_seeds, True, tile=tile, overlap=overlap, tile_condition=tile_condition,
                                       tile_fuse=tile_fuse, orientations=orientations)
            return EnsembleQuantiles(ens.mean, ens.std, ens.spread, ens.samples if return_samples else None,
                                     ensemble_quantiles(ens.samples, quantiles), quantiles)
        if tile is not None:
            return self._sample_ensemble_tiled(x_input, K, slice_seeds, return_samples, tile, overlap, tile_condition, tile_fuse)
        x01 = list(x_input)[0]
        codes = None
        if orientations is not None:                                     # the codes are checked before any work
            if not torch.is_tensor(x01) or x01.dim() != 4 or x01.shape[1] != 1:
                raise RuntimeError("sample_ensemble: x_input must be [ldct (B,1,H,W)]")
            codes = orientation_codes(orientations, K, x01.shape[2] == x01.shape[3])
        x01 = x01.contiguous().float()
        B = x01.shape[0]
        seeds = self._slice_seeds(slice_seeds, B, "cpu")
        rows = torch.from_numpy(ensemble_seeds(seeds.numpy(), K).reshape(-1)).to(x01.device)
        if codes is not None:
            return self._ensemble_oriented(x01, K, rows, codes, return_samples)
        return _ensemble_result(self._range_checked(lambda: self._ensemble_rows(x01, K, rows), "a sampled image"), return_samples)

    def _rows_final(self, x_rows, seeds, passes, x_T, cond=None):
        """The final images of the R rows x_rows (R,1,h,w) through _sample, in [0, 1] units: one call per pass (lo, hi) of `passes`,
        under the rows' seeds (R,) int64 on the device.  x_T is the rows' x_T noise: a row tensor (R,1,h,w), or a callable
        (a pass's seeds, its size) -> that pass's noise, drawn when the pass runs.  cond: the rows' preset conditioning
        (_cond_buffers), and x_rows are then in [-1, 1]; without it they are plain rows in [0, 1], which _sample normalises and
        whose tower it runs itself."""
        final = torch.empty(tuple(x_rows.shape), device=x_rows.device, dtype=torch.float32)
        for lo, hi in passes:
            sl = slice(lo, hi)
            sd = seeds[sl].contiguous()
            nz = x_T(sd, (hi - lo,) + tuple(x_rows.shape[1:])) if callable(x_T) else x_T[sl]
            pre = {} if cond is None else {"cond": self._cond_rows(cond, sl)}
            final[sl].copy_(self._sample([x_rows[sl]], hi - lo, True, nz, None, sd, **pre)[-1])
        return final

    def _ensemble_rows(self, x01, K, seeds):
        """The B K final images (B,K,1,H,W) of sample_ensemble; seeds (B K,) int64 on the device, row b K + k."""
        B, npix = x01.shape[0], x01[0].numel()
        x_n = self._normalize(x01)
        x_rows = self._engines()[0]._b("ens_xin", (B * K,) + tuple(x01.shape[1:]), torch.float32)
        L.call("fd_rows_repeat_f32", _p(x_n), _p(x_rows), B, K, npix, _stream(x01))
        cond = self._cond_repeated("ens", x_n, K, lambda u, e, x: e.encode_condition(x))
        # every plan's ancestral steps take the keyed stream of a pass's seeds inside its captured loop: no step_noise callable
        flat = self._rows_final(x_rows, seeds, ensemble_passes(B, K, self._group_rows()),
                                lambda sd, size: self._keyed_noise(sd, self.X_T_STEP, size), cond)
        return flat.view((B, K) + tuple(x01.shape[1:]))

    def _ensemble_oriented(self, x01, K, seeds, codes, return_samples):
        """sample_ensemble(orientations=...): see its docstring.  seeds (B K,) int64 on the device, row b K + k; codes (K,) int32 on
        the host, replica k's orientation."""
        B, _, H, W = x01.shape
        dev, s = x01.device, _stream(x01)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
        elem = np.asarray([orientation_inverse(orientation_inverse(c)) for c in codes])         # codes 8..15 as their 0..7 twins
        uniq, pos = np.unique(elem, return_inverse=True)                                         # D distinct orientations
        D = len(uniq)

        def oriented_rows():
            x_n = self._normalize(x01)
            x_rows = self._engines()[0]._b("ens_xin", (B * K, 1, H, W), torch.float32)
            L.call("fd_rows_orient_f32", _p(x_n), _p(x_rows), _p(up(codes)), B, K, H, W, s)
            # the tower on the B D distinct oriented inputs (row b D + d), at most max_sub_batch at a time; replica k of slice b
            # takes row b D + pos[k]
            x_tow = torch.empty((B * D, 1, H, W), device=dev, dtype=torch.float32)
            L.call("fd_rows_orient_f32", _p(x_n), _p(x_tow), _p(up(uniq)), B, D, H, W, s)
            tower, cond = self._cond_buffers("ori_tower", B * D), self._cond_buffers("ori", B * K)
            take = up((np.arange(B)[:, None] * D + pos[None, :]).reshape(-1))
            for e, (pe, la), (cpe, cla) in zip(self._engines(), tower, cond):
                for lo in range(0, B * D, self.max_sub_batch):
                    hi = min(lo + self.max_sub_batch, B * D)
                    e.encode_condition(x_tow[lo:hi])
                    pe[lo:hi].copy_(e.prompt_emb)
                    la[lo:hi].copy_(e.local_all)
                L.call("fd_rows_take_f32", _p(pe), _p(cpe), _p(take), B * K, e.time_dim, s)
                L.call("fd_rows_take_f32", _p(la), _p(cla), _p(take), B * K, e.loc_total, s)
            return self._rows_final(x_rows, seeds, ensemble_passes(B, K, self._group_rows()),
                                    lambda sd, size: self._keyed_noise(sd, self.X_T_STEP, size), cond)
        final = self._range_checked(oriented_rows, "a sampled image")
        nblk = L.lib().fd_ensemble_nblk(H * W)
        mean, std = torch.empty_like(x01), torch.empty_like(x01)
        ws, spread = torch.empty(B * nblk, device=dev), torch.empty(B, device=dev)
        samples = torch.empty((B, K, 1, H, W), device=dev, dtype=torch.float32) if return_samples else None
        L.call("fd_ensemble_orient_stats_f32", _p(final), _p(up([orientation_inverse(c) for c in codes])), _p(mean), _p(std), _p(ws),
               _p(spread), None if samples is None else _p(samples), B, K, H, W, s)
        return EnsembleResult(mean, std, spread, samples)

    def _sample_ensemble_tiled(self, x_input, K, slice_seeds, return_samples, tile, overlap, condition, fuse):
        """sample_ensemble(tile=...): see its docstring"""
        fn = "sample_ensemble"
        if fuse not in ("final", "step"):
            raise RuntimeError(f"{fn}: tile_fuse must be 'final' or 'step' (got {fuse!r})")
        x01, plan, seeds = TiledSampling._tiled_call(self, fn, x_input, tile, overlap, slice_seeds, condition, K)
        B, _, H, W = x01.shape
        dev = x01.device
        rseeds = torch.from_numpy(ensemble_seeds(seeds.numpy(), K).reshape(-1)).to(dev)                    # (B K,): a replica's
        rows = torch.from_numpy(tiled_ensemble_seeds(seeds.numpy(), K, plan.T).reshape(-1)).to(dev)         # (B K T,): a tile row's
        field = self._keyed_noise(rseeds, self.X_T_STEP, (B * K, 1, H, W))

        def replica_rows():
            x_n = self._normalize(x01)
            x_in = self._tile_gather(x_n, plan)
            return self._rows_per_replica(x_in, self._tile_cond_rows(x_n, x_in, plan, condition), B, K)
        if fuse == "step":
            def fused():
                x_rows, cond = replica_rows()
                img = self._x_T_into(x_rows, self._tile_gather(field, plan), torch.empty_like(x_rows))
                return self._tiled_fused_loop(x_rows, img, cond, rseeds, plan)
            return _ensemble_result(self._range_checked(fused, "a sampled image").view(B, K, 1, H, W), return_samples)

        def final_tiles():
            x_rows, cond = replica_rows()
            return self._rows_final(x_rows, rows, tile_passes(B * K, plan.my, plan.mx, self._group_rows(), self.streams),
                                    self._tile_gather(field, plan), cond)
        tiles = self._range_checked(final_tiles, "a sampled image (a tile row of a replica)")
        nblk = L.lib().fd_ensemble_nblk(H * W)
        mean, std = torch.empty_like(x01), torch.empty_like(x01)
        ws, spread = torch.empty(B * nblk, device=dev), torch.empty(B, device=dev)
        samples = torch.empty((B, K, 1, H, W), device=dev, dtype=torch.float32) if return_samples else None
        L.call("fd_tiles_ensemble_f32", _p(tiles), *plan.tables(), None if samples is None else _p(samples),
               _p(mean), _p(std), _p(ws), _p(spread), *plan.geometry(B, K), _stream(x01))
        return EnsembleResult(mean, std, spread, samples)

    # ---- a slice as overlapping tiles
    def _tile_plan(self, H, W, th, tw, oy, ox, dev):
        """The TilePlan of a geometry on `dev`, uploaded once"""
        cache = self.__dict__.setdefault("_tile_plans", {})
        key = (H, W, th, tw, oy, ox, str(dev))
        plan = cache.get(key)
        if plan is None:
            ys, xs = tile_plan(H, th, oy), tile_plan(W, tw, ox)
            up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a.astype(dt))).to(dev)
            plan = cache[key] = TilePlan(up(ys, np.int32), up(xs, np.int32), up(tile_weights(ys, H, th), np.float32),
                                         up(tile_weights(xs, W, tw), np.float32), len(ys), len(xs),
                                         int(bool((xs % 4 == 0).all())), th, tw, H, W)
        return plan

    def _tiled_args(self, fn, x_input, tile, overlap, condition):
        """The argument checks of a tiled call `fn`: (x01 as given, (th, tw), (oy, ox))"""
        if self.input_condition:
            raise RuntimeError(f"{fn}: input_condition=True is not built (one input plane per slice)")
        if condition not in ("tile", "slice"):
            raise RuntimeError(f"{fn}: condition must be 'tile' or 'slice' (got {condition!r})")
        (th, tw), (oy, ox) = tile_pair(fn, tile, "tile"), tile_pair(fn, overlap, "overlap")
        x01 = list(x_input)[0]
        if not torch.is_tensor(x01) or x01.dim() != 4 or x01.shape[1] != 1:
            raise RuntimeError(f"{fn}: x_input must be [ldct (B,1,H,W)]")
        B, _, H, W = x01.shape
        div = 2 ** (len(self.model.unet0.dim_mults) - 1)
        if th < 1 or tw < 1 or th % div or tw % div:
            raise RuntimeError(f"{fn}: tile {th} x {tw} must be positive multiples of {div} (the U-Net has "
                               f"{len(self.model.unet0.dim_mults)} levels)")
        if th > H or tw > W:
            raise RuntimeError(f"{fn}: tile {th} x {tw} is larger than the slice {H} x {W} (padded tiles are not built)")
        if not (0 <= oy <= th // 2 and 0 <= ox <= tw // 2):
            raise RuntimeError(f"{fn}: overlap {oy} x {ox} must lie in [0, tile // 2] = [0, {th // 2}] x [0, {tw // 2}]")
        return x01, (th, tw), (oy, ox)

    def _tiled_call(self, fn, x_input, tile, overlap, slice_seeds, condition, K=None):
        """The preamble of a tiled call `fn`: the argument checks, then (x01 fp32 and contiguous, its TilePlan, the slice seeds on the
        host).  K: the replicas per slice of a tiled ensemble, which count towards the row limit of the kernels' grids.
        (The callers take it unbound, as it takes _tiled_args: the host-side checks run on any object that has input_condition,
        tests/test_tiled_fused_cpu.py.)"""
        x01, (th, tw), (oy, ox) = TiledSampling._tiled_args(self, fn, x_input, tile, overlap, condition)
        B, _, H, W = x01.shape
        x01 = x01.contiguous().float()
        seeds = self._slice_seeds(slice_seeds, B, "cpu")
        plan = self._tile_plan(H, W, th, tw, oy, ox, x01.device)
        if B * (K or 1) * plan.T > 65535:
            replicas = "" if K is None else f"{K} replicas x "
            raise RuntimeError(f"{fn}: {B} slices x {replicas}{plan.my} x {plan.mx} tiles are more than 65535 rows: sample fewer "
                               "slices per call")
        return x01, plan, seeds

    @torch.no_grad()
    @_fuse_keyword
    def sample_tiled(self, x_input, tile, overlap=0, slice_seeds=None, condition="tile"):
        """x_input = [ldct (B,1,H,W) in [0,1]] sampled as overlapping tiles of `tile` = th or (th, tw) pixels, `overlap` (an int or
        a pair, at most tile // 2) pixels apart from full tiles (tiling.tile_plan: the last tile of an axis is shifted back to end
        at the border), and blended on the device: what sample(last=True) returns, [x_T image, final image], both (B,1,H,W).  A
        model trained on crops meets the operator it was trained under, an image larger than a checkpoint's size can be denoised,
        and the engines' workspaces are those of a tile.
        x_T is ONE keyed field per slice, fd_keyed_normal(slice seed, X_T_STEP) over the whole plane, and a tile's x_T noise is
        its window of that field: overlapping tiles start from the same noise in their common pixels, on both samplers.  The first
        returned image is x_input + sqrt(sum_scale) * field on the whole slice.  Tile (iy, ix) of slice b is an ordinary row of
        sample() under the seed tiling.tile_seeds(slice_seeds, my * mx)[b, iy * mx + ix] (tile 0 keeps the slice's seed: a one-tile
        plan is sample() of the slice under that x_T); the rows run slice-major in passes of at most streams x max_sub_batch
        through the paths of sample().  The ancestral sampler's STEP noise is the keyed stream of the tile's own seed (the
        graph-captured loop of every plan, the two-U-Net and pred_noise models included), so overlapping tiles see different step
        noise in their common pixels and the blend averages them.
        The final image is the weighted mean of the tiles' final images, weights tiling.tile_weights (fd_tiles_blend_f32): a
        pixel under one tile is that tile's value bit for bit.  Nothing returned depends on B or on the cut into passes.
        condition="tile": the DA-CLIP tower runs on every tile, which is what crop training saw.  "slice": it runs once per slice
        on the whole slice (Unet.tower_engine) and every tile of the slice takes those conditioning rows.
        `fuse` is a further, keyword-only argument (taken by _fuse_keyword in front of this method; an unknown value raises).
        fuse="final" (the default) is all of the above: every tile runs its own trajectory and the final images are blended once.
        fuse="step" fuses the tiles at EVERY step instead: the slice has one state x_t, held as tile rows that agree bit for bit
        in the common pixels of overlapping tiles.  Per step the forwards of all tile rows run into output buffers, in equal
        sub-batches of at most max_sub_batch rows per engine (half of it for a two-U-Net plan), each under its own conditioning
        rows (computed once before the loop, for both values of `condition`), and ONE launch of fd_tiles_step_ddim_f32 /
        fd_tiles_step_keyed_f32 blends the tiles' raw outputs per pixel (the weights and arithmetic of fd_tiles_blend_f32) and
        applies the scheduler update to every row in place; the ancestral step noise is the keyed stream of the SLICE seed at the
        slice pixel, the same for every covering tile (tile_seeds are not used).  It is one trajectory of the whole slice under a
        windowed model: the final image is assembled from the rows on the last step, every pixel being every covering tile's
        value, so there is no seam and no mean of different denoisings or noise realisations.  A one-tile plan is sample() of the
        two-U-Net and pred_noise plans bit for bit; the first returned image is that of fuse="final".  Every plan of _plan()
        runs, the shipped one as mode 0, on both samplers (_anc_max_chunks bounds the ancestral one as in _obj_ancestral), on one
        stream with slot 0's engines, eagerly: no captured graph, no second stream, and no precision tail for any plan -- a bf16
        fused run of the shipped plan does not get final_fp32_steps.  Nothing returned depends on B or on max_sub_batch.
        Ensembles of tiled samples are sample_ensemble(tile=...).  Not built: tiles larger than the slice (padded tiles),
        last=False, input_condition=True; for fuse="step" also a captured graph or a second stream, a precision tail, and
        per-tile seeds."""
        x01, plan, seeds = TiledSampling._tiled_call(self, "sample_tiled", x_input, tile, overlap, slice_seeds, condition)
        B, dev = x01.shape[0], x01.device
        rows = torch.from_numpy(tile_seeds(seeds.numpy(), plan.T).reshape(-1)).to(dev)
        field = self._keyed_noise(seeds.to(dev), self.X_T_STEP, tuple(x01.shape))
        x_T = self._x_T_into(self._normalize(x01), field, torch.empty_like(x01))
        if self._tile_fuse == "step":
            def fused():
                x_n = self._normalize(x01)
                x_in = self._tile_gather(x_n, plan)
                img = self._x_T_into(x_in, self._tile_gather(field, plan), torch.empty_like(x_in))
                cond = self._tile_cond_rows(x_n, x_in, plan, condition)
                return self._tiled_fused_loop(x_in, img, cond, seeds.to(dev), plan)
            return [self._unnormalize(x_T), self._range_checked(fused, "a sampled image")]
        tiles = self._range_checked(lambda: self._tile_rows(x01, field, rows, plan, condition), "a sampled image")
        out = torch.empty_like(x01)
        L.call("fd_tiles_blend_f32", _p(tiles), *plan.tables(), _p(out), *plan.geometry(B), _stream(x01))
        return [self._unnormalize(x_T), out]

    def _tile_gather(self, src, plan):
        """The B T tile rows (R,1,th,tw) of the B slices src (B,1,H,W)"""
        B = src.shape[0]
        dst = torch.empty((B * plan.T, 1, plan.th, plan.tw), device=src.device, dtype=torch.float32)
        L.call("fd_tiles_gather_f32", _p(src), _p(dst), _p(plan.ys), _p(plan.xs), *plan.geometry(B), _stream(src))
        return dst

    def _cond_buffers(self, prefix, R):
        """One (prompt_emb, local_all) pair of R conditioning rows per engine of _engines(), in buffers `prefix`_prompt /
        `prefix`_local of the engine whose rows they are (_encode_all and _cond_rows take the list)."""
        return [(e._b(prefix + "_prompt", (R, e.time_dim), torch.float32), e._b(prefix + "_local", (R, e.loc_total), torch.float32))
                for e in self._engines()]

    def _cond_repeated(self, prefix, x_n, n, encode):
        """_cond_buffers of the B n rows in which every slice of x_n (in [-1, 1]) stands n times: encode(unet, engine, slices)
        leaves the slices' conditioning in the engine, at most max_sub_batch slices at a time (the tower's workspace grows with its
        batch), on every engine in use, and a slice's rows are repeated for its n rows (replicas, tiles)."""
        B, s = x_n.shape[0], _stream(x_n)
        cond = self._cond_buffers(prefix, B * n)
        for c0 in range(0, B, self.max_sub_batch):
            nb = min(self.max_sub_batch, B - c0)
            for u, e, (pe, la) in zip(self._plan_unets(), self._engines(), cond):
                encode(u, e, x_n[c0:c0 + nb])
                L.call("fd_rows_repeat_f32", _p(e.prompt_emb), _p(pe[c0 * n:]), nb, n, e.time_dim, s)
                L.call("fd_rows_repeat_f32", _p(e.local_all), _p(la[c0 * n:]), nb, n, e.loc_total, s)
        return cond

    def _tile_cond_slice(self, x_n, T):
        """condition="slice": the conditioning rows of the B x T tile rows of the slices x_n.  The tower runs once per slice on
        the whole slice, on a tower-only engine per U-Net in use; the engine of the tiles turns its outputs into conditioning rows."""
        return self._cond_repeated("til", x_n, T, lambda u, e, x: e.condition_from(*u.tower_engine(e.mode).encode_dose(x)))

    def _fused_passes(self, B, plan):
        """The sub-batches of the B T tile rows that one engine takes at a time outside _sample: at most max_sub_batch rows,
        half of it for a two-U-Net plan."""
        return tile_passes(B, plan.my, plan.mx, max(1, self.max_sub_batch // 2 if self._plan().two_engines else self.max_sub_batch))

    def _tile_cond_rows(self, x_n, x_in, plan, condition):
        """The conditioning rows of the B T tile rows x_in (R,1,th,tw) gathered from the slices x_n (both in [-1, 1]), one
        (prompt_emb, local_all) pair per engine of _engines().  The tower runs once: on every tile (condition "tile", a
        sub-batch of _fused_passes at a time), or on the whole slices."""
        B = x_n.shape[0]
        if condition == "slice":
            return self._tile_cond_slice(x_n, plan.T)
        cond = self._cond_buffers("til", B * plan.T)
        for lo, hi in self._fused_passes(B, plan):
            for e, (pe, la) in zip(self._engines(), cond):
                e.encode_condition(x_in[lo:hi])
                pe[lo:hi].copy_(e.prompt_emb)
                la[lo:hi].copy_(e.local_all)
        return cond

    def _rows_per_replica(self, x_in, cond, B, K):
        """The input tiles and conditioning rows (_tile_cond_rows) of B slices, a slice's T rows repeated for its K replicas:
        row (b K + k) T + j = row b T + j (fd_rows_repeat_f32 with a row length of T times a row's)."""
        s = _stream(x_in)
        x_rows = torch.empty((x_in.shape[0] * K,) + tuple(x_in.shape[1:]), device=x_in.device, dtype=torch.float32)
        L.call("fd_rows_repeat_f32", _p(x_in), _p(x_rows), B, K, x_in.numel() // B, s)
        rows = self._cond_buffers("tens", x_in.shape[0] * K)
        for src, dst in zip(cond, rows):
            for a, b in zip(src, dst):
                L.call("fd_rows_repeat_f32", _p(a), _p(b), B, K, a.numel() // B, s)
        return x_rows, rows

    def _tiled_fused_loop(self, x_in, img, cond, seeds, plan):
        """One trajectory of B slices of H x W as R = B T tile rows (sample_tiled's docstring), given the rows' input tiles x_in,
        their x_T img (updated in place), their conditioning rows cond (_tile_cond_rows) and one seed per slice: sample_tiled
        hands in its slices' rows, sample_ensemble those of its B K replicas.  Per step: [fd_obj_begin on the ancestral sampler,]
        per U-Net of the plan and per sub-batch load_condition + forward into the rows of o0 / o1, then one fd_tiles_step_* launch
        over all R rows in place on img, which also writes the slice image on the last step."""
        B = x_in.shape[0] // plan.T
        dev, s = x_in.device, _stream(x_in)
        mode = self._plan().mode
        engines = self._engines()
        passes = self._fused_passes(B, plan)
        nmax = max(hi - lo for lo, hi in passes)
        outs = [torch.empty_like(x_in) for _ in engines]
        o0, o1 = self._o01(outs)
        final = torch.empty((B, 1, plan.H, plan.W), device=dev, dtype=torch.float32)
        geom = (*plan.tables(), *plan.geometry(B))

        def forwards(times):
            for e, o, tb, c in zip(engines, outs, times, cond):
                for lo, hi in passes:
                    e.load_condition(c[0][lo:hi], c[1][lo:hi])
                    e.forward(img[lo:hi], x_in[lo:hi], tb[:hi - lo], out=o[lo:hi])

        if self.is_ddim_sampling:
            S = self.sampling_timesteps
            par, tt0, tt1 = self._obj_ddim_table(nmax)
            gpar = par[:, 0].contiguous().to(dev)                  # (S, 8): all rows of a step share the parameters
            gts = [tt.to(dev) for tt in (tt0, tt1) if tt is not None]
            for i in range(S):
                forwards([gt[i] for gt in gts])
                L.call("fd_tiles_step_ddim_f32", mode, _p(o0), _p(o1), _p(img), _p(x_in), _p(gpar[i]), *geom, _p(img),
                       _p(final) if i == S - 1 else None, s)
        else:
            T = self.num_timesteps
            t_dev = torch.full((1,), T, device=dev, dtype=torch.int32)
            gpar = self._obj_anc_table().to(dev)
            tabs = [None if tt is None else tt.to(dev) for tt in self._obj_time_tables()]
            bufs = [None if tt is None else torch.zeros(nmax, device=dev, dtype=torch.float32) for tt in tabs]
            G, reps, rem = self._anc_chunks(T)                     # _obj_ancestral's steps under _anc_max_chunks
            steps = rem + reps * G
            for i in range(steps):
                L.call("fd_obj_begin", _p(t_dev), _p(tabs[0]), _p(tabs[1]), _p(bufs[0]), _p(bufs[1]), nmax, T, s)
                forwards([b for b in bufs if b is not None])
                L.call("fd_tiles_step_keyed_f32", mode, _p(o0), _p(o1), _p(img), _p(x_in), _p(gpar), _p(t_dev), _p(seeds), *geom,
                       _p(img), _p(final) if i == steps - 1 else None, T, s)
            self._anc_steps_run = steps
        return self._unnormalize(final)

    def _tile_rows(self, x01, field, seeds, plan, condition):
        """The B T final tile images (R,1,th,tw) of sample_tiled, in [0, 1] units; seeds (R,) int64 on the device."""
        B = x01.shape[0]
        nz_rows = self._tile_gather(field, plan)
        cond = None
        if condition == "slice":
            x_n = self._normalize(x01)                             # the rows of a preset are already in [-1, 1] (_sample)
            x_rows = self._tile_gather(x_n, plan)
            cond = self._tile_cond_slice(x_n, plan.T)
        else:
            x_rows = self._tile_gather(x01, plan)                  # plain rows of _sample, which normalises them itself
        return self._rows_final(x_rows, seeds, tile_passes(B, plan.my, plan.mx, self._group_rows(), self.streams), nz_rows, cond)
