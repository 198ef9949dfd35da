"""CT slice I/O, the normalisation contract, the mixed-dose datasets on either side of the sampling path, and a paired dataset held
on the GPU (DeviceSliceStore) whose batches a HIP kernel gathers and augments (csrc/fd_train_data.hip) or cuts to patches first
(csrc/fd_train_crop.hip).

Reference contract:
  * slices are `.npy` arrays in HU + 1024, stored (1, H, W) (`ToTensor(expand_dims=False)` asserts ndim 3,
    /root/reference/data/transforms.py:618-634); `Normalize`: x = clip((m - 1024 + 1000) / 3000, 0, 1)
    (data/transforms.py:572-587), float32;
  * a test item is the pair [NDCT (target), LDCT (condition)]  (data/pdf_dataset.py:424-466): the low-dose file
    `<loc>-...-<dose>-<index>.npy` names its anatomy (`loc` = head | lung | ab) and the index of its full-dose
    partner in that anatomy's NDCT list; the last '-' token of both file names must agree;
  * dose labels (data/pdf_dataset.py:480-510, data/dose_dataset.py:101-129): full_1mm -> 1, quarter_1mm -> 4
    (10 for lung in the test set), simulated dose fraction 0.5 / 0.33 / 0.25 / 0.20 / 0.17 / 0.12 / 0.10 / 0.05 ->
    2 / 3 / 4 / 5 / 6 / 8 / 10 / 20;
  * results are saved as np.save(<name[:-4]>, out.reshape(H, W)) in [0,1]  (src/DADiff.py:1913-1914);
  * previews use the HU window clip(x*3000-1000, -160, 240), (x+160)/400  (src/DADiff.py:1794-1795) and
    torchvision's save_image grid.
The reference's datasets glob hard-coded private paths inside their constructors; here the file lists are
arguments, everything else (pairing, labels, names, normalisation) follows the reference.
"""
import os

import numpy as np
import torch

from . import _lib as L
from ._train import empty, ptr, stream

DOSE_LABELS = {0.5: 2, 0.33: 3, 0.25: 4, 0.20: 5, 0.17: 6, 0.12: 8, 0.10: 10, 0.05: 20}


def normalize_hu(m, min_value=-1000.0, max_value=2000.0):
    """transforms.Normalize (data/transforms.py:572-587): stored value - 1024 -> [0, 1]."""
    m = np.asarray(m, dtype=np.float32) - 1024.0
    return np.clip((m - min_value) / (max_value - min_value), 0.0, 1.0).astype(np.float32)


def to_tensor(m, expand_dims=False):
    """transforms.ToTensor (data/transforms.py:618-634)."""
    assert m.ndim in (3, 4), "Supports only 3D (DxHxW) or 4D (CxDxHxW) images"
    if expand_dims and m.ndim == 3:
        m = np.expand_dims(m, axis=0)
    return torch.from_numpy(m.astype(np.float32))


def load_slice(path):
    """One stored slice -> (1, H, W) float32 tensor in [0, 1].  Accepts the reference's (1, H, W) arrays and
    plain (H, W) ones."""
    m = np.load(path).astype(np.float32)
    if m.ndim == 2:
        m = m[None]
    return to_tensor(normalize_hu(m))


def save_slice(path, x01):
    """The inverse storage rule (HU + 1024, (1, H, W) float32) -- used to write test volumes."""
    x = np.asarray(x01, dtype=np.float32).reshape((1,) + tuple(np.asarray(x01).shape[-2:]))
    np.save(path, x * 3000.0 - 1000.0 + 1024.0)


def hu_window(x01, lo=-160.0, hi=240.0):
    """[0,1]-normalised image -> display window in [0,1] (torch tensor or ndarray)."""
    if isinstance(x01, torch.Tensor):
        return (torch.clip(x01 * 3000 - 1000, lo, hi) - lo) / (hi - lo)
    return (np.clip(x01 * 3000 - 1000, lo, hi) - lo) / (hi - lo)


def define_label(path, lung_quarter_is_10=True):
    """Dose label of a file path.  `lung_quarter_is_10`: the test dataset's rule (data/pdf_dataset.py:486-490);
    False gives the Dose-CLIP training dataset's (data/dose_dataset.py:106-108).  That dataset has no branch for
    the 0.25 fraction -- its `label` stays unbound there -- so the same path raises here too."""
    if "full_1mm" in path:
        return 1
    if "quarter_1mm" in path:
        return 10 if (lung_quarter_is_10 and "lung" in path) else 4
    dose = float(path.split("-")[-2])
    if dose == 0.25 and not lung_quarter_is_10:
        raise UnboundLocalError("local variable 'label' referenced before assignment "
                                "(data/dose_dataset.py:110-126 has no branch for dose 0.25)")
    if dose not in DOSE_LABELS:
        raise UnboundLocalError(f"no dose label for fraction {dose} in {path!r}")
    return DOSE_LABELS[dose]


def make_grid(t, nrow=8, padding=2, pad_value=0.0):
    """torchvision.utils.make_grid for a (B, C, H, W) tensor (the reference's preview layout)."""
    t = t.detach().float().cpu()
    if t.dim() == 3:
        t = t[None]
    if t.shape[1] == 1:
        t = t.repeat(1, 3, 1, 1)
    B, C, H, W = t.shape
    xmaps = min(nrow, B)
    ymaps = (B + xmaps - 1) // xmaps
    hh, ww = H + padding, W + padding
    grid = t.new_full((C, hh * ymaps + padding, ww * xmaps + padding), pad_value)
    for k in range(B):
        y, x = divmod(k, xmaps)
        grid[:, y * hh + padding:y * hh + padding + H, x * ww + padding:x * ww + padding + W] = t[k]
    return grid


def save_image(t, path, nrow=8):
    """torchvision.utils.save_image: grid -> clamp [0,1] -> *255 + 0.5 -> uint8 PNG (src/DADiff.py:1812)."""
    from PIL import Image
    g = make_grid(t, nrow=nrow)
    arr = g.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(torch.uint8).numpy()
    Image.fromarray(arr).save(path)


class CTSliceDataset(torch.utils.data.Dataset):
    """Pairs of (low-dose, normal-dose) `.npy` slices -> [NDCT, LDCT] tensors (1,H,W) in [0,1]."""

    def __init__(self, ldct_paths, ndct_paths):
        assert len(ldct_paths) == len(ndct_paths)
        self.q_path_list, self.f_path_list = list(ldct_paths), list(ndct_paths)

    def __len__(self):
        return len(self.q_path_list)

    def __getitem__(self, i):
        return [load_slice(self.f_path_list[i]), load_slice(self.q_path_list[i])]

    def load_name(self, index, sub_dir=False):
        return os.path.basename(self.q_path_list[index])


class MixedDoseTestDataset(torch.utils.data.Dataset):
    """The reference's test dataset (data/pdf_dataset.py:424-510): a flat list of low-dose slices of several
    anatomies and dose levels, each paired with its full-dose partner through the file name.

    q_paths: low-dose files `<loc>-<...>-<dose>-<index>.npy` (loc = head | lung | ab);
    ndct_paths: {loc: sorted list of that anatomy's full-dose files}."""

    def __init__(self, q_paths, ndct_paths):
        self.q_path_list = list(q_paths)
        self.ndct = {k: list(v) for k, v in ndct_paths.items()}
        self.A_size = len(self.q_path_list)
        self.dataset_size = [len(self.ndct.get(k, [])) for k in ("ab", "lung", "head")]

    def __len__(self):
        return self.A_size

    def partner(self, index):
        path = self.q_path_list[index]
        loc = path.split("/")[-1].split("-")[0]
        ndct_index = int(path.split(".")[-2].split("-")[-1])
        if loc not in self.ndct:
            raise KeyError(f"no full-dose list for anatomy {loc!r} ({path})")
        f = self.ndct[loc][ndct_index]
        assert f.split("-")[-1] == path.split("-")[-1], (f, path)
        return f

    def __getitem__(self, index):
        return [load_slice(self.partner(index)), load_slice(self.q_path_list[index])]

    def load_name(self, index, sub_dir=False):
        name = self.q_path_list[index]
        if sub_dir == 0:
            return os.path.basename(name)
        return os.path.dirname(name).split("/")[-1] + "_" + os.path.basename(name)

    def define_label(self, path):
        return define_label(path, lung_quarter_is_10=True)

    def dose(self, index):
        """1 / label: the dose fraction feature of data/pdf_dataset.py:452."""
        return 1.0 / self.define_label(self.q_path_list[index])


class DoseDataset(torch.utils.data.Dataset):
    """The Dose-CLIP dataset's item layout and label scheme (data/dose_dataset.py:80-129): every slice of every
    dose level (full-dose first, then 1/2 ... 1/20), item = ([x, x], label) with x (1,H,W) in [0,1] and label the
    dose denominator as float32.  `images_list`: the concatenated per-dose file lists."""

    def __init__(self, images_list):
        self.images_list = list(images_list)

    def __len__(self):
        return len(self.images_list)

    def define_label(self, path):
        return define_label(path, lung_quarter_is_10=False)

    def __getitem__(self, index):
        path = self.images_list[index]
        x = load_slice(path)
        return [x, x.clone()], np.asarray(self.define_label(path)).astype(np.float32)


def shard_indices(n, world, rank):
    """Contiguous block of the item range for this rank (founddiff_amd.parallel.shard_range): how a mixed-dose
    volume is split over the GPUs of a node."""
    from .parallel import shard_range
    lo, hi = shard_range(n, world, rank)
    return list(range(lo, hi))


class SyntheticCTDataset(torch.utils.data.Dataset):
    """Seeded phantoms (founddiff_amd.synth.ct_phantom) with the same item layout; five noise levels cycle
    through the items like a mixed-dose list."""

    def __init__(self, n, size, seed=10):
        from .synth import ct_phantom
        self.nd, self.ld = ct_phantom(n, size, seed)

    def __len__(self):
        return self.nd.shape[0]

    def __getitem__(self, i):
        return [torch.from_numpy(self.nd[i]), torch.from_numpy(self.ld[i])]

    def load_name(self, index, sub_dir=False):
        return f"synthetic-quarter-{index:04d}.npy"


def upload_table(rows, device):
    """the int64 rows as one (len(rows), B) table on the device: one copy from pinned memory on the current stream, not waited
    for (torch's pinned allocator keeps the block until the copy has left it)"""
    tab = torch.from_numpy(np.ascontiguousarray(np.stack([np.asarray(r, dtype=np.int64) for r in rows])))
    return tab.pin_memory().to(device, non_blocking=True)


def crop_pair(fn, crop, name="crop"):
    """`crop` as (ch, cw): an int, or an (h, w) pair of integers"""
    is_int = lambda v: isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))
    c = (crop, crop) if is_int(crop) else crop
    if not (isinstance(c, (tuple, list)) and len(c) == 2 and all(is_int(v) for v in c)):
        raise RuntimeError(f"{fn}: {name} must be an int or an (h, w) pair of integers (got {crop!r})")
    return int(c[0]), int(c[1])


def crop_pads(n, c):
    """(before, after): the reflect padding of an axis of length n cropped to c >= n (CropToFixed, data/transforms.py:196-249)"""
    before = max(c - n, 0) // 2
    return before, max(c - n, 0) - before


def window_rows(windows):
    """the (B, 2) windows as two rows of a batch's (rows, B) table: side by side they are the (B, 2) array again"""
    return list(np.ascontiguousarray(windows, dtype=np.int64).reshape(2, -1))


def check_batch(fn, store, indices, codes, windows=None, crop=None):
    """(indices, codes, windows, crop) of a batch from `store`: int64 arrays (codes and windows None stay None) and crop as
    (ch, cw) or None: types, then shapes, then ranges"""
    if not isinstance(store, DeviceSliceStore):
        raise RuntimeError(f"{fn}: store must be a DeviceSliceStore (got {type(store).__name__})")
    out = []
    for name, v in (("indices", indices), ("codes", codes), ("windows", windows)):
        if v is None and name != "indices":
            out.append(None)
            continue
        if isinstance(v, torch.Tensor):
            v = v.detach().cpu().numpy()
        try:
            a = np.asarray(v)
        except Exception:
            a = None
        if a is not None and a.size == 0:
            a = a.astype(np.int64)                       # an empty list has no dtype of its own: its shape is what is wrong
        if a is None or a.dtype.kind not in "iu":
            raise RuntimeError(f"{fn}: {name} must be a sequence of integers (got {type(v).__name__}"
                               f"{'' if a is None else ' of ' + str(a.dtype)})")
        out.append(a.astype(np.int64))
    idx, cd, win = out
    if crop is not None:
        crop = crop_pair(fn, crop)
    elif win is not None:
        raise RuntimeError(f"{fn}: windows need a crop (got crop=None)")
    if idx.ndim != 1 or idx.size < 1 or (cd is not None and cd.shape != idx.shape):
        raise RuntimeError(f"{fn}: inconsistent shapes indices{idx.shape} codes{None if cd is None else cd.shape} (both (B,), B >= 1)")
    if win is not None and win.shape != (idx.size, 2):
        raise RuntimeError(f"{fn}: inconsistent shapes indices{idx.shape} windows{win.shape} (windows (B, 2): y0, x0 per item)")
    if idx.size > 65535:
        raise RuntimeError(f"{fn}: unsupported shape indices{idx.shape} (at most 65535 slices)")
    H, W = store.H, store.W
    if crop is not None:
        ch, cw = crop
        if not (1 <= ch <= 32768 and 1 <= cw <= 32768):
            raise RuntimeError(f"{fn}: unsupported shape crop {ch} x {cw} (1 <= h, w <= 32768)")
        if crop_pads(H, ch)[1] > H - 1 or crop_pads(W, cw)[1] > W - 1:
            raise RuntimeError(f"{fn}: unsupported shape crop {ch} x {cw} of {H} x {W} slices (one reflection only: a pad of at most "
                               f"{H - 1} rows and {W - 1} columns on either side)")
    if idx.min() < 0 or idx.max() >= len(store):
        raise RuntimeError(f"{fn}: index {int(idx[(idx < 0) | (idx >= len(store))][0])} outside [0, {len(store)})")
    if cd is not None:
        if cd.min() < 0 or cd.max() >= 16:
            raise RuntimeError(f"{fn}: code {int(cd[(cd < 0) | (cd >= 16)][0])} outside [0, 16)")
        if crop is None and H != W and (cd & 4).any():
            raise RuntimeError(f"{fn}: code {int(cd[(cd & 4) != 0][0])} transposes (k odd), the store's slices are {H} x {W}")
        if crop is not None and crop[0] != crop[1] and (cd & 4).any():
            raise RuntimeError(f"{fn}: code {int(cd[(cd & 4) != 0][0])} transposes (k odd), the crop is {crop[0]} x {crop[1]}")
    if win is not None:
        ny, nx = max(H - crop[0], 1), max(W - crop[1], 1)
        bad = (win[:, 0] < 0) | (win[:, 0] >= ny) | (win[:, 1] < 0) | (win[:, 1] >= nx)
        if bad.any():
            y0, x0 = (int(v) for v in win[bad][0])
            raise RuntimeError(f"{fn}: window ({y0}, {x0}) outside [0, {ny}) x [0, {nx}) (a {crop[0]} x {crop[1]} crop of {H} x {W} slices)")
    return idx, cd, win, crop


class DeviceSliceStore:
    """A paired dataset on the GPU in the form load_slice returns (fp32 in [0, 1], normalised on the host): nd (n_nd, H, W),
    ld (n_ld, H, W) and nd_index (n_ld,) int64, on the host (nd_index) and on the device (nd_index_dev): item i is the pair
    [nd[nd_index[i]], ld[i]], so several dose levels share one stored NDCT.  It has the dataset surface (__len__,
    __getitem__ -> device views, load_name), so it also serves as `dataset=` of Trainer.sample / test; batch() gathers a batch
    under the flip / rot90 codes of diffusion_train.train_augment in one launch (fd_store_gather_f32; cut to the windows of
    diffusion_train.train_crop first with crop=: fd_store_crop_f32), and diffusion_train.StoreBatch hands one to the training step
    without assembling it."""

    def __init__(self, nd, ld, nd_index, names=None):
        fn = "DeviceSliceStore"
        for name, v in (("nd", nd), ("ld", ld)):
            if not isinstance(v, torch.Tensor):
                raise RuntimeError(f"{fn}: {name} must be a tensor (got {type(v).__name__})")
            if v.dtype != torch.float32:
                raise RuntimeError(f"{fn}: {name} must be float32 (got {v.dtype})")
        idx = nd_index.detach().cpu().numpy() if isinstance(nd_index, torch.Tensor) else np.asarray(nd_index)
        if idx.dtype.kind not in "iu":
            raise RuntimeError(f"{fn}: nd_index must hold integers (got {idx.dtype})")
        idx = idx.astype(np.int64)
        if names is not None and not (isinstance(names, (list, tuple)) and all(isinstance(n, str) for n in names)):
            raise RuntimeError(f"{fn}: names must be a list of strings")
        shapes = f"nd{tuple(nd.shape)} ld{tuple(ld.shape)} nd_index{idx.shape}"
        if nd.dim() != 3 or ld.dim() != 3 or nd.shape[1:] != ld.shape[1:] or idx.shape != (ld.shape[0],) or \
                (names is not None and len(names) != ld.shape[0]):
            raise RuntimeError(f"{fn}: inconsistent shapes {shapes} (nd (n_nd, H, W), ld (n_ld, H, W), nd_index and names (n_ld,))")
        if nd.numel() < 1 or ld.numel() < 1:
            raise RuntimeError(f"{fn}: the dataset is empty ({shapes})")
        if nd.shape[1] > 32768 or nd.shape[2] > 32768:
            raise RuntimeError(f"{fn}: unsupported shape {shapes} (H, W <= 32768)")
        if idx.min() < 0 or idx.max() >= nd.shape[0]:
            raise RuntimeError(f"{fn}: nd_index points outside nd ({shapes})")
        for name, v in (("nd", nd), ("ld", ld)):
            if not v.is_cuda:
                raise RuntimeError(f"{fn}: {name} must live on the GPU (there is no CPU path)")
        if ld.device != nd.device:
            raise RuntimeError(f"{fn}: ld lives on {ld.device}, nd on {nd.device}")
        self.nd, self.ld, self.nd_index = nd.contiguous(), ld.contiguous(), idx
        self.nd_index_dev = torch.from_numpy(idx).to(nd.device)
        self.names = None if names is None else list(names)
        self.n_nd, self.n_ld, self.H, self.W = nd.shape[0], ld.shape[0], nd.shape[1], nd.shape[2]
        self.device = nd.device

    # ---- constructors: everything is checked on the host before the first upload
    @staticmethod
    def _device(fn, device):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError(f"{fn}: the store must live on the GPU (there is no CPU path; got device {dev})")
        return dev

    @staticmethod
    def _slice(fn, v, what):
        if isinstance(v, np.ndarray):
            v = torch.from_numpy(v)
        if not isinstance(v, torch.Tensor):
            raise RuntimeError(f"{fn}: {what} must be a tensor (got {type(v).__name__})")
        if v.dim() == 3 and v.shape[0] == 1:
            v = v[0]
        if v.dim() != 2 or v.numel() < 1:
            raise RuntimeError(f"{fn}: unsupported shape {what}{tuple(v.shape)} (a slice is (1, H, W) or (H, W))")
        return v.float()

    @classmethod
    def _from_slices(cls, fn, nd, ld, nd_index, names, device):
        if not ld:
            raise RuntimeError(f"{fn}: the dataset is empty")
        shapes = {tuple(v.shape) for v in nd} | {tuple(v.shape) for v in ld}
        if len(shapes) != 1:
            raise RuntimeError(f"{fn}: mixed slice shapes {sorted(shapes)} (a store holds slices of one shape)")
        dev = cls._device(fn, device)

        def upload(rows, chunk=256):
            out = torch.empty((len(rows),) + tuple(rows[0].shape), device=dev, dtype=torch.float32)
            for s in range(0, len(rows), chunk):
                out[s:s + chunk].copy_(torch.stack(rows[s:s + chunk]))
            return out
        return cls(upload(nd), upload(ld), np.asarray(nd_index, dtype=np.int64), names)

    @classmethod
    def from_items(cls, items, device):
        """a list of [ndct, ldct] pairs ((1, H, W) or (H, W) each); one NDCT is stored per item"""
        fn = "DeviceSliceStore.from_items"
        if not isinstance(items, (list, tuple)):
            raise RuntimeError(f"{fn}: items must be a list of [ndct, ldct] pairs (got {type(items).__name__})")
        nd, ld = [], []
        for k, it in enumerate(items):
            if not isinstance(it, (list, tuple)) or len(it) != 2:
                raise RuntimeError(f"{fn}: item {k} must be [ndct, ldct] (got {type(it).__name__})")
            nd.append(cls._slice(fn, it[0], f"item {k}'s ndct"))
            ld.append(cls._slice(fn, it[1], f"item {k}'s ldct"))
        return cls._from_slices(fn, nd, ld, range(len(ld)), None, device)

    @classmethod
    def from_dataset(cls, ds, device):
        """any object with __len__ and __getitem__ -> [ndct, ldct]; one NDCT is stored per item, load_name is kept if present"""
        fn = "DeviceSliceStore.from_dataset"
        if not hasattr(ds, "__len__") or not hasattr(ds, "__getitem__"):
            raise RuntimeError(f"{fn}: ds must have __len__ and __getitem__ (got {type(ds).__name__})")
        nd, ld = [], []
        for k in range(len(ds)):
            it = ds[k]
            if not isinstance(it, (list, tuple)) or len(it) != 2:
                raise RuntimeError(f"{fn}: item {k} must be [ndct, ldct] (got {type(it).__name__})")
            nd.append(cls._slice(fn, it[0], f"item {k}'s ndct"))
            ld.append(cls._slice(fn, it[1], f"item {k}'s ldct"))
        names = [ds.load_name(k) for k in range(len(ds))] if hasattr(ds, "load_name") else None
        return cls._from_slices(fn, nd, ld, range(len(ld)), names, device)

    @classmethod
    def from_mixed_dose(cls, ds, device):
        """a MixedDoseTestDataset: every full-dose file is stored once, however many dose levels name it as their partner"""
        fn = "DeviceSliceStore.from_mixed_dose"
        if not isinstance(ds, MixedDoseTestDataset):
            raise RuntimeError(f"{fn}: ds must be a MixedDoseTestDataset (got {type(ds).__name__})")
        slots, nd, ld, nd_index = {}, [], [], []
        for k in range(len(ds)):
            f = ds.partner(k)
            if f not in slots:
                slots[f] = len(nd)
                nd.append(cls._slice(fn, load_slice(f), f"the partner of item {k}"))
            nd_index.append(slots[f])
            ld.append(cls._slice(fn, load_slice(ds.q_path_list[k]), f"item {k}"))
        return cls._from_slices(fn, nd, ld, nd_index, [ds.load_name(k) for k in range(len(ds))], device)

    # ---- the dataset surface
    def __len__(self):
        return self.n_ld

    def __getitem__(self, i):
        i = int(i)
        if not 0 <= i < self.n_ld:
            raise IndexError(f"DeviceSliceStore: index {i} outside [0, {self.n_ld})")
        return [self.nd[int(self.nd_index[i])][None], self.ld[i][None]]

    def load_name(self, index, sub_dir=False):
        return self.names[index] if self.names is not None else f"store-quarter-{int(index):06d}.npy"

    @property
    def nbytes(self):
        return 4 * (self.nd.numel() + self.ld.numel()) + 8 * self.n_ld

    def batch(self, indices, codes=None, windows=None, crop=None):
        """(x_start, x_input), both (B, 1, H, W): items `indices` under the transform `codes` (diffusion_train.train_augment;
        None: as stored), in one launch.  A transposing code (k odd) needs square slices.
        crop (an int or (h, w)): the reference's CropToFixed first, then the transform on the crop; both results are
        (B, 1, h, w).  windows (B, 2) = (y0, x0) per item (diffusion_train.train_crop; None: zeros), each inside
        [0, max(H - h, 1)) x [0, max(W - w, 1)); an axis no longer than the crop is taken whole and reflect-padded to it, once:
        a pad of at most H - 1 / W - 1 on either side.  A transposing code then needs a square crop, whatever the slices are."""
        idx, cd, win, crop = check_batch("DeviceSliceStore.batch", self, indices, codes, windows, crop)
        B = len(idx)
        with torch.no_grad(), torch.cuda.device(self.device):
            rows = [self.nd_index[idx], idx] + ([] if cd is None else [cd])
            at = len(rows)
            tab = upload_table(rows + ([] if win is None else window_rows(win)), self.device)
            new = empty(self.device)
            codes_ptr = None if cd is None else ptr(tab[2])
            if crop is None:
                x_start, x_input = new(B, 1, self.H, self.W), new(B, 1, self.H, self.W)
                L.call("fd_store_gather_f32", ptr(self.nd), ptr(self.ld), self.n_nd, self.n_ld, ptr(tab[0]), ptr(tab[1]), codes_ptr,
                       ptr(x_start), ptr(x_input), B, self.H, self.W, stream(self.device))
            else:
                x_start, x_input = new(B, 1, *crop), new(B, 1, *crop)
                L.call("fd_store_crop_f32", ptr(self.nd), ptr(self.ld), self.n_nd, self.n_ld, ptr(tab[0]), ptr(tab[1]), codes_ptr,
                       None if win is None else ptr(tab[at]), ptr(x_start), ptr(x_input), B, self.H, self.W, crop[0], crop[1],
                       stream(self.device))
        return x_start, x_input
