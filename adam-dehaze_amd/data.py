"""Input side of the hot path on device: the reference's synthetic fog model as one HIP kernel, a synthetic
foggy-frame loader that never leaves the GPU, and image folders served from a device-resident 8-bit cache.

/root/reference utils/helpers.py:201-265 (`apply_random_fog`) converts every image to numpy, draws (beta, A) with
`np.random.uniform`, builds the depth map and the transmission in float64 and loops over the channels on the host.
Here the draws stay on the host in the reference's order (so `np.random.seed(s)` reproduces its parameters), and
`I = clip(J*t + A*(1-t))` runs in `adh_apply_fog` for the whole batch.  `synthetic_loader` stands in for the DataLoader
with the same batch dict keys when no image folders are configured.

Image folders (data/dataset.py:9-124, 233-249 of the reference): `folder_index` lists the hazy / clear pairs of a split,
`FolderDataset` decodes every file once on host threads (Pillow), brings it to `img_size` once on the GPU
(`adh_u8_resize_bilinear`) and keeps the split as two dense uint8 [L,H,W,3] device tensors; `FolderDataset.epoch` yields the
batch dicts, each image batch assembled by `adh_batch_from_u8` (v / 255 and the train transform in one gather pass over 3
bytes per pixel).  `epoch_plan` is the pure host function that decides which samples a rank sees in which order;
`folder_loader` is what the drivers call.  With `dataset.crop_size` the files keep their own sizes in two flat uint8 tensors
and a batch is random (train) or centre crops of them, assembled by `adh_batch_window_from_u8` from a byte offset and a row
pitch per sample (`batch_from_windows`, `draw_crop_origins`, `centre_origins`, `upscaled_size`).  There are no worker processes and no streaming loader: a split that does not fit
in half of the free device memory is refused.

Clear images plus depth maps (`dataset.synthetic_haze`, the RESIDE recipe): `haze_index` lists `<split>/clear/<name>` with
`depth/<stem>.png`, `HazeSynthDataset` keeps the clear bytes and a uint16 depth cache on the device, and `batch_haze_from_windows`
renders the hazy role of every batch from them (`adh_batch_haze_from_u8`: the scattering model at source pixels, then the paired
transform), under a fresh (label, beta, A) per sample and epoch from `draw_haze_params`.  With `nonuniform` / `chromatic` in that
section the renderer is `batch_nhhaze_from_windows` (`adh_batch_nhhaze_from_u8`): patchy haze from a noise field anchored to the
image and beta, A per channel, drawn by `draw_nh_params` after the former.
"""
from __future__ import annotations

import copy
import os
from concurrent.futures import ThreadPoolExecutor
from typing import Callable, Dict, Iterator, List, Mapping, Optional, Sequence, Union

import numpy as np
import torch

from . import _hip as H

# helpers.py:222-234
FOG_RANGES = {"low": ((0.1, 0.4), (0.5, 0.7)), "medium": ((0.4, 0.7), (0.7, 0.9)), "high": ((0.7, 1.0), (0.8, 1.0)),
              "random": ((0.1, 1.0), (0.5, 1.0))}
LEVEL_NAMES = ("low", "medium", "high")


def apply_fog(clear: torch.Tensor, beta: torch.Tensor, airlight: torch.Tensor) -> torch.Tensor:
    """hazy[n] = clip(clear[n]*t_n + A_n*(1 - t_n), 0, 1), t_n = exp(-beta_n * depth) (helpers.py:241-258);
    clear [N,3,H,W] float32 in [0,1] on the GPU, beta / airlight [N]."""
    H.require_cuda(clear, "clear image batch")
    if clear.dim() != 4 or clear.shape[1] != 3:
        raise RuntimeError(f"expected [N,3,H,W], got {tuple(clear.shape)}")
    clear = clear.contiguous()
    N, _, Hh, Ww = clear.shape
    beta = beta.to(device=clear.device, dtype=torch.float32).contiguous()
    airlight = airlight.to(device=clear.device, dtype=torch.float32).contiguous()
    if beta.numel() != N or airlight.numel() != N:
        raise RuntimeError("beta / airlight must have one entry per image")
    hazy = torch.empty_like(clear)
    H.call("adh_apply_fog", clear.data_ptr(), beta.data_ptr(), airlight.data_ptr(), N, Hh, Ww, hazy.data_ptr())
    return hazy


def draw_fog_params(intensities: Sequence[str], rng=None):
    """(beta, A) per image, drawn like helpers.py:237-238: np.random.uniform(*beta_range) then
    np.random.uniform(*A_range), image after image.  `rng`: anything with .uniform (default: the global np.random)."""
    rng = np.random if rng is None else rng
    betas, As = [], []
    for name in intensities:
        (b0, b1), (a0, a1) = FOG_RANGES.get(name, FOG_RANGES["random"])
        betas.append(rng.uniform(b0, b1))
        As.append(rng.uniform(a0, a1))
    return torch.tensor(betas, dtype=torch.float64), torch.tensor(As, dtype=torch.float64)


def apply_random_fog(clear_img: torch.Tensor, intensity: Union[str, Sequence[str]] = "random", rng=None) -> torch.Tensor:
    """helpers.py:201-265 for GPU tensors: [N,3,H,W] or [3,H,W] in [0,1] (values > 1 are taken as 0..255 and scaled,
    as the reference does); `intensity` one name for all images or one per image."""
    single = clear_img.dim() == 3
    x = clear_img.unsqueeze(0) if single else clear_img
    if float(x.max()) > 1.0:
        x = x / 255.0
    names = [intensity] * x.shape[0] if isinstance(intensity, str) else list(intensity)
    beta, A = draw_fog_params(names, rng)
    out = apply_fog(x.float(), beta, A)
    return out[0] if single else out


def draw_augment_params(n: int, rng=None) -> torch.Tensor:
    """[n, 5] float32 {flip_h, flip_v, brightness_first, b, c}: the random choices of the reference's training transform
    (data/dataset.py:59-64: RandomHorizontalFlip, RandomVerticalFlip, ColorJitter(brightness=0.1, contrast=0.1)) for n
    samples, drawn the way data/dataset.py:100-116 does: `seed = np.random.randint(2147483647)` per sample, then
    `torch.manual_seed(seed)` before the transform of EACH of the sample's images -- so hazy / clear / dehazed get the same
    choices, which is why one parameter row per sample suffices.  Draw order inside the transform (torchvision):
    `torch.rand(1) < 0.5` (horizontal), `torch.rand(1) < 0.5` (vertical), `torch.randperm(4)` (order of brightness /
    contrast / saturation / hue; the last two are off), `uniform(0.9, 1.1)` for brightness, then for contrast."""
    rng = np.random if rng is None else rng
    rows = []
    for _ in range(n):
        g = torch.Generator().manual_seed(int(rng.randint(2147483647)))
        fh = float(torch.rand(1, generator=g) < 0.5)
        fv = float(torch.rand(1, generator=g) < 0.5)
        perm = torch.randperm(4, generator=g).tolist()
        b = float(torch.empty(1).uniform_(0.9, 1.1, generator=g))
        c = float(torch.empty(1).uniform_(0.9, 1.1, generator=g))
        rows.append([fh, fv, float(perm.index(0) < perm.index(1)), b, c])
    return torch.tensor(rows, dtype=torch.float32)


def paired_augment(images: Sequence[torch.Tensor], params: Optional[torch.Tensor] = None, rng=None):
    """Apply ONE set of per-sample choices (`draw_augment_params`) to every tensor of `images` ([N,3,H,W] float32 in
    [0,1] on the GPU: hazy, clear, dehazed ...), on device.  Returns (list of augmented tensors, params)."""
    x0 = images[0]
    H.require_cuda(x0, "image batch")
    N, Cc, Hh, Ww = x0.shape
    if Cc != 3:
        raise RuntimeError(f"expected [N,3,H,W], got {tuple(x0.shape)}")
    if params is None:
        params = draw_augment_params(N, rng)
    pd = params.to(device=x0.device, dtype=torch.float32).contiguous()
    nblk = H.value("adh_augment_num_blocks", Hh * Ww)
    outs = []
    for x in images:
        if x.shape != x0.shape:
            raise RuntimeError("paired images must have one shape")
        H.require_cuda(x, "image batch")
        x = x.contiguous()
        partial = torch.empty(N * nblk, device=x.device, dtype=torch.float64)
        out = torch.empty_like(x)
        H.call("adh_paired_augment", x.data_ptr(), pd.data_ptr(), N, Hh, Ww, partial.data_ptr(), nblk, out.data_ptr())
        outs.append(out)
    return outs, params


def synthetic_loader(batch_size: int, size, steps: int, seed: int = 42, rank: int = 0,
                     device: Optional[torch.device] = None, augment: bool = False) -> Iterator[Dict]:
    """Foggy / clear pairs with the reference's fog model, generated on `device` (default cuda): low-pass random clear
    frames, labels uniform in {0,1,2}, (beta, A) from the label's range.  Batch dict keys as data/dataset.py:118-124
    ('dehazed' omitted: nothing on the path reads it)."""
    import torch.nn.functional as F
    h, w = (size, size) if isinstance(size, int) else size
    device = torch.device("cuda") if device is None else torch.device(device)
    g = torch.Generator(device=device).manual_seed(seed + 1000 * rank)
    host = np.random.RandomState(seed + 1000 * rank)
    for _ in range(steps):
        clear = torch.rand(batch_size, 3, h, w, generator=g, device=device)
        clear = F.avg_pool2d(F.pad(clear, (2, 2, 2, 2), mode="reflect"), 5, 1)
        labels = torch.from_numpy(host.randint(0, 3, size=batch_size).astype(np.int64))
        beta, A = draw_fog_params([LEVEL_NAMES[int(i)] for i in labels], host)
        hazy = apply_fog(clear, beta, A)
        if augment:     # the reference's train-split transform, same choices for both images of a pair
            (hazy, clear), _ = paired_augment([hazy, clear], rng=host)
        yield {"hazy": hazy, "clear": clear, "intensity": labels.to(device),
               "name": [f"synthetic_{i}" for i in range(batch_size)]}


# ---------------------------------------------------------------------------------------------------------------- image folders
IMAGE_SUFFIXES = (".jpg", ".png")      # data/dataset.py:37, case-sensitive
MAX_DECODE_THREADS = 16


class FolderIndex(list):
    """the records of `folder_index`, plus `skipped` (hazy files without a clear file of the same name) and `split_dir`"""
    skipped = 0
    split_dir = ""


def _split_dir(root: str, split: str) -> Optional[str]:
    """the directory that holds {low,medium,high}/hazy for `split`: <root>/<split>, else <root> itself, else None"""
    if not root:
        return None
    for d in (os.path.join(root, split), root):
        if any(os.path.isdir(os.path.join(d, level, "hazy")) for level in LEVEL_NAMES):
            return d
    return None


def folder_index(root: str, split: str) -> Optional[FolderIndex]:
    """The samples of one split as records {hazy, clear, intensity, name}, or None when there are no image folders.

    Layout of data/dataset.py:20-52: `<root>/<split>/{low,medium,high}/{hazy,clear}/<name>`, labels low 0, medium 1, high 2.
    When `<root>/<split>` holds no `<level>/hazy` directory but `<root>` does, `<root>` itself is the split directory (with
    `--data_dir D` the reference's path handling asks for `D/train/train`, and no dataset is laid out like that).  Names
    must end in `.jpg` or `.png` (case-sensitive, the reference's rule); each level's names are sorted (the reference takes
    `os.listdir` order, which is arbitrary).  A hazy file without a clear file of the same name is skipped and counted in
    the result's `skipped`.  Deviation from the reference: the `dehazed` folder is neither required nor read (the reference
    lists a sample only when hazy, clear and dehazed all exist; nothing on the path reads `dehazed`, see `synthetic_loader`).
    None: no `<level>/hazy` directory exists under either candidate, e.g. a root that holds only `annotations/`."""
    d = _split_dir(root, split)
    if d is None:
        return None
    out = FolderIndex()
    out.split_dir = d
    for label, level in enumerate(LEVEL_NAMES):
        hazy_dir, clear_dir = os.path.join(d, level, "hazy"), os.path.join(d, level, "clear")
        if not os.path.isdir(hazy_dir):
            continue
        for name in sorted(os.listdir(hazy_dir)):
            if not name.endswith(IMAGE_SUFFIXES):
                continue
            hazy, clear = os.path.join(hazy_dir, name), os.path.join(clear_dir, name)
            if not os.path.isfile(hazy):
                continue
            if not os.path.isfile(clear):
                out.skipped += 1
                continue
            out.append({"hazy": hazy, "clear": clear, "intensity": label, "name": name})
    return out


def epoch_plan(M: int, world: int, rank: int, batch_size: int, seed: int, epoch: int, train: bool) -> List[np.ndarray]:
    """The batches of one epoch on one rank, as int64 arrays of sample numbers 0..M-1 of the index.  Rank r owns the samples
    r, r + world, ...

    train: the rank's shard, padded by repeating its own first samples up to ceil(M / world), in the order of
    `np.random.RandomState(seed + epoch).permutation`; every rank so yields ceil(ceil(M / world) / batch_size) batches (the
    gradient all-reduce is per step: a rank with one batch fewer would leave the others waiting).  Otherwise: the shard in
    index order, no padding and no repeats, so a metric counts every file once; a rank may have one sample fewer, or none.
    The last batch may be short (the reference's drop_last=False)."""
    if M < 1 or world < 1 or not 0 <= rank < world or batch_size < 1:
        raise ValueError(f"epoch_plan: M={M}, world={world}, rank={rank}, batch_size={batch_size}")
    own = np.arange(rank, M, world, dtype=np.int64)
    if train:
        if own.size == 0:
            raise ValueError(f"epoch_plan: rank {rank} of {world} has no sample of its own among {M}: train on fewer ranks")
        own = np.resize(own, -(-M // world))
        own = own[np.random.RandomState(seed + epoch).permutation(own.size)]
    return [own[i:i + batch_size] for i in range(0, own.size, batch_size)]


def batch_from_cache(cache, index: torch.Tensor, params: Optional[torch.Tensor] = None):
    """Images `index` of a dense uint8 [M,H,W,3] device cache as float32 [N,3,H,W], each value exactly v / 255; with `params`
    ([N,5] rows of `draw_augment_params`) the train transform of `paired_augment` is applied in the same pass.  `cache` may be
    a sequence of caches of one shape (hazy, clear): the result is then a list, one batch per cache, from ONE upload of the
    index and of the parameter rows, so the roles of a pair get the same samples and the same choices.  `index` is a CPU
    int64 tensor: it is checked against 0 <= index < M here, on the host, before anything touches the device (IndexError),
    because the kernel does not validate it; there is no entry point that takes a device index."""
    caches = [cache] if isinstance(cache, torch.Tensor) else list(cache)
    if not isinstance(index, torch.Tensor) or index.is_cuda or index.dtype != torch.int64 or index.dim() != 1:
        raise TypeError("batch_from_cache: index must be a 1-D int64 tensor on the CPU")
    c0 = caches[0]
    for c in caches:
        if c.dim() != 4 or c.shape[3] != 3 or c.shape != c0.shape:
            raise ValueError(f"batch_from_cache: the caches must be [M,H,W,3] of one shape, got {[tuple(c.shape) for c in caches]}")
    M, Hh, Ww, _ = c0.shape
    N = index.numel()
    if N < 1:
        raise ValueError("batch_from_cache: empty index")
    if int(index.min()) < 0 or int(index.max()) >= M:
        raise IndexError(f"batch_from_cache: index out of range for a cache of {M} images: {index.tolist()}")
    for c in caches:
        if not c.is_cuda or c.dtype != torch.uint8 or not c.is_contiguous() or c.device != c0.device:
            raise RuntimeError(f"adam-dehaze_amd: the cache must be a dense uint8 tensor on one cuda device, got {c.dtype} on "
                               f"{c.device} (no CPU fallback)")
    if params is not None and tuple(params.shape) != (N, 5):
        raise ValueError(f"batch_from_cache: params must be [{N},5], got {tuple(params.shape)}")
    nblk = H.value("adh_batch_num_blocks", Hh * Ww)
    outs = []
    with torch.cuda.device(c0.device):
        idx = index.contiguous().to(c0.device)
        pd = None if params is None else params.to(device=c0.device, dtype=torch.float32).contiguous()
        for c in caches:
            partial = None if pd is None else torch.empty(N * nblk, device=c0.device, dtype=torch.float64)
            out = torch.empty((N, 3, Hh, Ww), device=c0.device, dtype=torch.float32)
            H.call("adh_batch_from_u8", c.data_ptr(), Hh * Ww * 3, M, Hh, Ww, idx.data_ptr(), H.ptr(pd), N, H.ptr(partial), nblk,
                   out.data_ptr())
            outs.append(out)
    return outs[0] if isinstance(cache, torch.Tensor) else outs


def batch_from_windows(cache, windows: torch.Tensor, crop, params: Optional[torch.Tensor] = None):
    """`crop` = (CH, CW) windows of a flat uint8 device cache that holds images of any sizes, as float32 [N,3,CH,CW] of exactly
    v / 255: row y of sample n is the CW * 3 interleaved RGB bytes at `cache[windows[n,0] + y * windows[n,1]:]`, so `windows` (CPU
    int64 [N,2]) holds the byte offset of each window's first pixel and its image's row pitch (`crop_windows`).  With `params`
    the train transform is applied in the same pass, the grey mean of the contrast step taken over the window: bit for bit
    `batch_from_cache` on a dense copy of the windows' bytes.  `cache` may be a sequence of flat caches of one length (hazy,
    clear): one upload of the windows and of the rows then serves all of them and the result is a list.  The windows are checked
    here, on the host, before anything touches the device, because the kernel does not validate them: IndexError unless
    offset >= 0, pitch >= CW * 3 and offset + (CH - 1) * pitch + CW * 3 <= cache.numel() in every row."""
    caches = [cache] if isinstance(cache, torch.Tensor) else list(cache)
    if not isinstance(windows, torch.Tensor) or windows.is_cuda or windows.dtype != torch.int64 or windows.dim() != 2 \
            or windows.shape[1] != 2:
        raise TypeError("batch_from_windows: windows must be an int64 [N,2] tensor on the CPU")
    CH, CW = _size2(crop)
    if CH < 1 or CW < 1:
        raise ValueError(f"batch_from_windows: crop must be at least 1 x 1, got {(CH, CW)}")
    c0 = caches[0]
    for c in caches:
        if c.dim() != 1 or c.shape != c0.shape:
            raise ValueError(f"batch_from_windows: the caches must be flat and of one length, got {[tuple(c.shape) for c in caches]}")
    N = windows.shape[0]
    if N < 1:
        raise ValueError("batch_from_windows: no windows")
    if params is not None and tuple(params.shape) != (N, 5):
        raise ValueError(f"batch_from_windows: params must be [{N},5], got {tuple(params.shape)}")
    if any(o < 0 or p < CW * 3 or o + (CH - 1) * p + CW * 3 > c0.numel() for o, p in windows.tolist()):    # Python ints: no wrap
        raise IndexError(f"batch_from_windows: a {CH}x{CW} window leaves a cache of {c0.numel()} bytes: {windows.tolist()}")
    for c in caches:
        if not c.is_cuda or c.dtype != torch.uint8 or not c.is_contiguous() or c.device != c0.device:
            raise RuntimeError(f"adam-dehaze_amd: the cache must be a dense uint8 tensor on one cuda device, got {c.dtype} on "
                               f"{c.device} (no CPU fallback)")
    nblk = H.value("adh_batch_num_blocks", CH * CW)
    outs = []
    with torch.cuda.device(c0.device):
        wd = windows.contiguous().to(c0.device)
        pd = None if params is None else params.to(device=c0.device, dtype=torch.float32).contiguous()
        for c in caches:
            partial = None if pd is None else torch.empty(N * nblk, device=c0.device, dtype=torch.float64)
            out = torch.empty((N, 3, CH, CW), device=c0.device, dtype=torch.float32)
            H.call("adh_batch_window_from_u8", c.data_ptr(), c.numel(), wd.data_ptr(), H.ptr(pd), N, CH, CW, H.ptr(partial), nblk,
                   out.data_ptr())
            outs.append(out)
    return outs[0] if isinstance(cache, torch.Tensor) else outs


def crop_windows(offsets, sizes, origins) -> torch.Tensor:
    """int64 [n,2] rows {byte offset of the window's first pixel, row pitch} for `batch_from_windows`: images of `sizes` [n,2]
    (heights, widths) stored as dense interleaved RGB at byte `offsets` [n] of a flat cache, cropped at `origins` [n,2] (y0, x0)."""
    offsets, sizes, origins = (np.asarray(a, dtype=np.int64) for a in (offsets, sizes, origins))
    return torch.from_numpy(np.stack([offsets + (origins[:, 0] * sizes[:, 1] + origins[:, 1]) * 3, sizes[:, 1] * 3], axis=1))


def draw_crop_origins(sizes, crop, rng) -> np.ndarray:
    """int64 [n,2] random crop origins (y0, x0) for images of `sizes` [n,2] (heights, widths), uniform over the positions at
    which a `crop` = (CH, CW) window lies inside the image.  Per sample, in order: rng.randint(0, H - CH + 1), then
    rng.randint(0, W - CW + 1)."""
    CH, CW = _size2(crop)
    return np.array([[rng.randint(0, int(h) - CH + 1), rng.randint(0, int(w) - CW + 1)] for h, w in np.asarray(sizes)],
                    dtype=np.int64).reshape(-1, 2)


def centre_origins(sizes, crop) -> np.ndarray:
    """int64 [n,2]: ((H - CH) // 2, (W - CW) // 2), the centre crop of validation"""
    CH, CW = _size2(crop)
    return (np.asarray(sizes, dtype=np.int64).reshape(-1, 2) - np.array([CH, CW], dtype=np.int64)) // 2


def upscaled_size(h: int, w: int, crop) -> tuple:
    """The size at which an h x w image is cached for `crop` = (CH, CW) windows: its own when the crop fits inside it, otherwise
    the smallest size of its aspect ratio that holds one crop (the free side rounded half up, in integers)."""
    CH, CW = _size2(crop)
    if h >= CH and w >= CW:
        return int(h), int(w)
    if CH * w >= CW * h:
        return CH, max(CW, (2 * w * CH + h) // (2 * h))
    return max(CH, (2 * h * CW + w) // (2 * w)), CW


def _size2(img_size) -> tuple:
    h, w = (img_size, img_size) if isinstance(img_size, int) else img_size
    return int(h), int(w)


class FolderDataset:
    """One split of an image-folder dataset, resident on `device` as 8-bit pixels: `hazy` and `clear` uint8 [L,H,W,3], `labels`
    (int64 [L], device) and `names`, for this rank's shard of `records` (samples rank, rank + world, ... of the index).

    Every file is decoded once with `image_io.load_image` on `threads` host threads (at most 16; `dataset.num_workers` in the
    drivers), uploaded, and brought to `img_size` (int or [h, w]) by `adh_u8_resize_bilinear`, which also replicates grey and
    drops alpha.  A file that cannot be read raises, naming the path.  A cache that would take more than half of the free
    device memory raises: a streaming loader is not built.

    `crop_size` (int or [h, w]; `dataset.crop_size` in the drivers) keeps every pair at its own resolution instead and serves
    crops of that size: `hazy` and `clear` are then two flat uint8 tensors, pair k's images dense [sizes[k,0], sizes[k,1], 3]
    at byte `offsets[k]` (a multiple of 4; `sizes` int64 [L,2] and `offsets` int64 [L] stay on the host).  The sizes come from
    the files' headers before anything is decoded; a pair whose hazy and clear sizes differ raises.  A pair smaller than the
    crop on either side is cached at `upscaled_size`; every other file's bytes pass through.  `img_size` is not used then."""

    def __init__(self, records: Sequence[Dict], img_size, device, rank: int = 0, world: int = 1, threads: int = 4,
                 split: str = "train", crop_size=None):
        from .image_io import load_image
        self.H, self.W = _size2(img_size)
        self.crop = None if crop_size is None else _size2(crop_size)
        self.device = torch.device(device)
        self.rank, self.world, self.total = rank, world, len(records)
        own = list(records[rank::world])
        self.names = [r["name"] for r in own]
        L = len(own)
        nthreads = max(1, min(int(threads), MAX_DECODE_THREADS))
        if self.crop is None:
            shape, what, advice = (L, self.H, self.W, 3), f"{self.H}x{self.W}", "a smaller dataset.img_size"
        else:
            upscaled = self._layout(own, nthreads)
            shape, advice = (self.cache_bytes,), "a smaller dataset"
            what = f"their own sizes ({upscaled} upscaled to hold a {self.crop[0]}x{self.crop[1]} crop)"
        need = 2 * int(np.prod(shape, dtype=np.int64))
        if self.device.type != "cuda":
            raise RuntimeError(f"adam-dehaze_amd: the dataset cache lives on a cuda device, got {self.device} (no CPU fallback)")
        free = torch.cuda.mem_get_info(self.device)[0]
        if need > free // 2:
            raise RuntimeError(f"the {split} split needs {need} bytes of device memory as an 8-bit cache ({L} pairs at "
                               f"{what}), more than half of the {free} bytes free on {self.device}; a streaming "
                               f"loader is not built: use {advice} or more ranks")
        self.hazy = torch.empty(shape, dtype=torch.uint8, device=self.device)
        self.clear = torch.empty_like(self.hazy)
        self.labels = torch.tensor([r["intensity"] for r in own], dtype=torch.int64).to(self.device)

        def decode(job):
            try:
                return load_image(job[2])
            except Exception as e:
                raise RuntimeError(f"cannot read image file {job[2]}: {e}") from e
        jobs = [(cache, slot, r[role]) for slot, r in enumerate(own) for role, cache in (("hazy", self.hazy), ("clear", self.clear))]
        with ThreadPoolExecutor(nthreads) as pool, torch.cuda.device(self.device):
            for at in range(0, len(jobs), 4 * nthreads):        # a few files per thread in flight: decoded files do not pile up
                chunk = jobs[at:at + 4 * nthreads]
                for (cache, slot, path), img in zip(chunk, pool.map(decode, chunk)):
                    h, w, c = img.shape
                    src = img.contiguous().to(self.device)
                    if self.crop is None:
                        dst, oh, ow = cache[slot].data_ptr(), self.H, self.W
                    else:
                        (oh, ow), dst = self.sizes[slot].tolist(), cache.data_ptr() + int(self.offsets[slot])
                    H.call("adh_u8_resize_bilinear", src.data_ptr(), w * c, h, w, c, dst, oh, ow)
        print(f"Loaded {self.total} samples for {split} split")
        print(f"  skipped {getattr(records, 'skipped', 0)} hazy files without a clear file of the same name")
        print(f"  device cache: {L} pairs at {what} on {self.device}, {need / 2 ** 20:.1f} MiB"
              + (f" ({need} bytes)" if self.crop is not None else "") + (f" (rank {rank} of {world})" if world > 1 else ""))

    def _layout(self, own: Sequence[Dict], nthreads: int) -> int:
        """crop mode: `sizes`, `offsets` and `cache_bytes` (per role) from the files' headers; returns the number of pairs that
        are cached larger than their files"""
        from .image_io import _pil

        def header(path):
            try:
                with _pil().open(path) as im:       # reads the header, decodes nothing
                    w, h = im.size
            except Exception as e:
                raise RuntimeError(f"cannot read image file {path}: {e}") from e
            return int(h), int(w)
        with ThreadPoolExecutor(nthreads) as pool:
            hazy = list(pool.map(header, [r["hazy"] for r in own]))
            clear = list(pool.map(header, [r["clear"] for r in own]))
        sizes, offsets, at, upscaled = [], [], 0, 0
        for r, hs, cs in zip(own, hazy, clear):
            if hs != cs:
                raise ValueError(f"the files of a pair differ in size: {r['hazy']} is {hs[0]}x{hs[1]}, {r['clear']} is "
                                 f"{cs[0]}x{cs[1]}")
            size = upscaled_size(hs[0], hs[1], self.crop)
            upscaled += size != hs
            sizes.append(size)
            offsets.append(at)
            at += -(-size[0] * size[1] * 3 // 4) * 4             # every slot starts on a multiple of 4
        self.sizes = np.array(sizes, dtype=np.int64).reshape(-1, 2)
        self.offsets = np.array(offsets, dtype=np.int64)
        self.cache_bytes = at
        return upscaled

    def __len__(self):
        return len(self.names)

    def epoch(self, epoch: int, batch_size: int, seed: int, train: bool, augment: bool = True) -> Iterator[Dict]:
        """The batch dicts of `synthetic_loader` ('hazy', 'clear' float32 [n,3,H,W]; 'intensity' int64 [n], device; 'name' file
        names) in the order of `epoch_plan`.  train and `augment`: one `draw_augment_params` row per sample from this loader's
        own RandomState(seed + 1000 * rank + epoch); the same device rows drive hazy and clear.  In crop mode the images are
        [n,3,CH,CW]: a train batch draws, after its parameter rows (when `augment`), `draw_crop_origins` from the same
        RandomState, so every epoch sees fresh patches; every other batch takes the centre windows and no rows."""
        if self.total == 0 or (not train and len(self) == 0):
            return
        rng = np.random.RandomState(seed + 1000 * self.rank + epoch)
        for samples in epoch_plan(self.total, self.world, self.rank, batch_size, seed, epoch, train):
            index = torch.from_numpy((samples - self.rank) // self.world)
            params = draw_augment_params(index.numel(), rng) if train and augment else None
            if self.crop is None:
                hazy, clear = batch_from_cache((self.hazy, self.clear), index, params)
            else:
                sizes = self.sizes[index.numpy()]
                origins = draw_crop_origins(sizes, self.crop, rng) if train else centre_origins(sizes, self.crop)
                windows = crop_windows(self.offsets[index.numpy()], sizes, origins)
                hazy, clear = batch_from_windows((self.hazy, self.clear), windows, self.crop, params)
            yield {"hazy": hazy, "clear": clear, "intensity": self.labels[index.to(self.device)],
                   "name": [self.names[i] for i in index.tolist()]}


# ---------------------------------------------------------------------------------------------------------------- haze synthesis
DEPTH_SOURCES = ("folder", "radial")
DEFAULT_DEPTH_RANGE = (0.3, 1.0)      # the span of the reference's radial depth map (helpers.py:247)


def draw_haze_params(n: int, rng):
    """(labels int64 [n], fog float32 [n,2] = {beta, A}) for n synthesized samples.  Per sample, in order: `rng.randint(0, 3)` (the
    density label), then beta and A from `FOG_RANGES[LEVEL_NAMES[label]]` in `draw_fog_params`' order."""
    labels, fog = [], []
    for _ in range(n):
        label = int(rng.randint(0, 3))
        beta, A = draw_fog_params([LEVEL_NAMES[label]], rng)
        labels.append(label)
        fog.append([float(beta[0]), float(A[0])])
    return torch.tensor(labels, dtype=torch.int64), torch.tensor(fog, dtype=torch.float32).reshape(n, 2)


def fixed_haze_params(seed: int, samples):
    """`draw_haze_params` for evaluation: sample number g of the index (not of a shard) draws from RandomState((seed, g)) and from
    nothing else, so its (label, beta, A) are the same in every epoch, on every rank and for every world size."""
    drawn = [draw_haze_params(1, np.random.RandomState((int(seed) % 2 ** 32, int(g)))) for g in samples]
    return torch.cat([d[0] for d in drawn]), torch.cat([d[1] for d in drawn])


def fixed_nh_params(seed: int, samples, nonuniform, chromatic, sizes, origins):
    """`fixed_haze_params` plus the extras of `draw_nh_params`, drawn from the same RandomState((seed, g)) after the sample's
    (label, beta, A): -> (labels, fog [n,2], fog6 [n,6], field [n,6]), the same in every epoch, on every rank, for every world"""
    sizes = np.asarray(sizes, dtype=np.int64).reshape(-1, 2)
    origins = np.zeros_like(sizes) if origins is None else np.asarray(origins, dtype=np.int64).reshape(-1, 2)
    labels, fog, fog6, field = [], [], [], []
    for i, g in enumerate(samples):
        rng = np.random.RandomState((int(seed) % 2 ** 32, int(g)))
        lab, f2 = draw_haze_params(1, rng)
        f6, fld = draw_nh_params(1, rng, nonuniform, chromatic, sizes[i:i + 1], origins[i:i + 1], f2)
        labels.append(lab), fog.append(f2), fog6.append(f6), field.append(fld)
    return torch.cat(labels), torch.cat(fog), torch.cat(fog6), torch.cat(field)


def batch_haze_from_windows(clear: torch.Tensor, depth: Optional[torch.Tensor], geom: torch.Tensor, fog: torch.Tensor, crop,
                            params: Optional[torch.Tensor] = None, depth_range=DEFAULT_DEPTH_RANGE) -> torch.Tensor:
    """The hazy role of a batch rendered from clear pixels: float32 [N,3,CH,CW] = augment(fog(window)) by `adh_batch_haze_from_u8`.
    `clear` is a dense uint8 device tensor of interleaved RGB (the flat cache of crop mode or [M,H,W,3]), `depth` a dense uint16
    device tensor (flat or [M,H,W]) or None for the reference's radial depth over the window.  `geom` (CPU int64 [N,4], bytes):
    {clear offset of the window's first pixel, clear row pitch, depth offset, depth row pitch}; the last two are ignored without
    `depth`.  `fog` float32 [N,2] = {beta, A} (`draw_haze_params`), on the CPU or already on the cache's device.  Per pixel
    t = exp(-beta * d) in float64 with d = near + (far - near) * level / 65535 (`depth_range` = (near, far)), hazy =
    clamp(J * t + A * (1 - t)); with `params` the train transform follows in the same pass, its grey mean taken over the hazed
    window.  Everything is checked here, on the host, before anything touches the device, because the kernel does not validate
    `geom`: TypeError for a wrong index type, ValueError for an odd depth offset or pitch or a depth pitch below CW * 2,
    IndexError when a window leaves either cache, RuntimeError for a cache that is not on a cuda device."""
    if not isinstance(geom, torch.Tensor) or geom.is_cuda or geom.dtype != torch.int64 or geom.dim() != 2 or geom.shape[1] != 4:
        raise TypeError("batch_haze_from_windows: geom must be an int64 [N,4] tensor on the CPU")
    if not isinstance(clear, torch.Tensor) or (depth is not None and not isinstance(depth, torch.Tensor)):
        raise TypeError("batch_haze_from_windows: the caches must be tensors")
    CH, CW = _size2(crop)
    if CH < 1 or CW < 1:
        raise ValueError(f"batch_haze_from_windows: crop must be at least 1 x 1, got {(CH, CW)}")
    N = geom.shape[0]
    if N < 1:
        raise ValueError("batch_haze_from_windows: no windows")
    if not isinstance(fog, torch.Tensor) or tuple(fog.shape) != (N, 2):
        raise ValueError(f"batch_haze_from_windows: fog must be a [{N},2] tensor of (beta, A)")
    if params is not None and tuple(params.shape) != (N, 5):
        raise ValueError(f"batch_haze_from_windows: params must be [{N},5], got {tuple(params.shape)}")
    near, far = (float(v) for v in depth_range)
    if not (np.isfinite(near) and np.isfinite(far)):
        raise ValueError(f"batch_haze_from_windows: depth_range must be finite, got {depth_range}")
    rows = geom.tolist()                                                                                    # Python ints: no wrap
    if depth is not None and any(do % 2 or dp % 2 or dp < CW * 2 for _, _, do, dp in rows):
        raise ValueError(f"batch_haze_from_windows: depth offsets and pitches must be even and a pitch at least {CW * 2} bytes: "
                         f"{rows}")
    cbytes = clear.numel() * clear.element_size()
    if any(o < 0 or p < CW * 3 or o + (CH - 1) * p + CW * 3 > cbytes for o, p, _, _ in rows):
        raise IndexError(f"batch_haze_from_windows: a {CH}x{CW} window leaves a clear cache of {cbytes} bytes: {rows}")
    dbytes = 0 if depth is None else depth.numel() * depth.element_size()
    if depth is not None and any(do < 0 or do + (CH - 1) * dp + CW * 2 > dbytes for _, _, do, dp in rows):
        raise IndexError(f"batch_haze_from_windows: a {CH}x{CW} window leaves a depth cache of {dbytes} bytes: {rows}")
    for c, dt in ((clear, torch.uint8), (depth, torch.uint16)):
        if c is not None and (not c.is_cuda or c.dtype != dt or not c.is_contiguous() or c.device != clear.device):
            raise RuntimeError(f"adam-dehaze_amd: the cache must be a dense {dt} tensor on one cuda device, got {c.dtype} on "
                               f"{c.device} (no CPU fallback)")
    nblk = H.value("adh_batch_num_blocks", CH * CW)
    with torch.cuda.device(clear.device):
        gd = geom.contiguous().to(clear.device)
        fd = fog.to(device=clear.device, dtype=torch.float32).contiguous()
        pd = None if params is None else params.to(device=clear.device, dtype=torch.float32).contiguous()
        partial = None if pd is None else torch.empty(N * nblk, device=clear.device, dtype=torch.float64)
        out = torch.empty((N, 3, CH, CW), device=clear.device, dtype=torch.float32)
        H.call("adh_batch_haze_from_u8", clear.data_ptr(), cbytes, H.ptr(depth), dbytes, gd.data_ptr(), fd.data_ptr(), near, far,
               H.ptr(pd), N, CH, CW, H.ptr(partial), nblk, out.data_ptr())
    return out


# patchy, wavelength-dependent haze: `nonuniform` / `chromatic` of dataset.synthetic_haze
NH_DEFAULTS = {"nonuniform": {"amplitude": (0.2, 0.8), "cell": (0.15, 0.5), "octaves": 3},
               "chromatic": {"angstrom": (0.0, 1.3), "tint": 0.05}}
NH_MAX_OCTAVES = 4
NH_WAVELENGTHS_NM = (610.0, 550.0, 465.0)      # r, g, b; green keeps the drawn beta


def _nh_settings(which: str, value, where: str = "dataset.synthetic_haze") -> Optional[Dict]:
    """`nonuniform` / `chromatic` as given (None: off; True or {}: the defaults; a mapping: defaults overridden) -> a checked dict
    of plain floats / ints, or None.  ValueError names the key."""
    if value is None or value is False:
        return None
    defaults = NH_DEFAULTS[which]
    if value is True:
        value = {}
    if not isinstance(value, Mapping):
        raise ValueError(f"{where}.{which} must be a mapping with keys {sorted(defaults)}, got {value!r}")
    unknown = sorted(set(value) - set(defaults))
    if unknown:
        raise ValueError(f"{where}.{which}: unknown keys {unknown} (known: {', '.join(sorted(defaults))})")

    def pair(key, lo_min, hi_max, hi_open=False):
        v = value.get(key, defaults[key])
        ok = isinstance(v, (list, tuple)) and len(v) == 2 and all(isinstance(t, (int, float)) and not isinstance(t, bool) for t in v)
        if ok:
            lo, hi = float(v[0]), float(v[1])
            ok = np.isfinite(lo) and np.isfinite(hi) and lo_min <= lo <= hi and (hi < hi_max if hi_open else hi <= hi_max)
        if not ok:
            raise ValueError(f"{where}.{which}.{key} must be [lo, hi] with {lo_min} <= lo <= hi {'<' if hi_open else '<='} "
                             f"{hi_max}, got {v!r}")
        return (lo, hi)
    if which == "nonuniform":
        amplitude = pair("amplitude", 0.0, 1.0, hi_open=True)
        cell = pair("cell", 2.0 ** -20, 2.0 ** 20)
        if cell[0] <= 0:
            raise ValueError(f"{where}.{which}.cell must be [lo, hi] with 0 < lo <= hi, got {value.get('cell')!r}")
        K = value.get("octaves", defaults["octaves"])
        if isinstance(K, bool) or not isinstance(K, int) or not 1 <= K <= NH_MAX_OCTAVES:
            raise ValueError(f"{where}.{which}.octaves must be an integer in 1..{NH_MAX_OCTAVES}, got {K!r}")
        return {"amplitude": amplitude, "cell": cell, "octaves": int(K)}
    angstrom = pair("angstrom", -4.0, 4.0)
    tint = value.get("tint", defaults["tint"])
    if isinstance(tint, bool) or not isinstance(tint, (int, float)) or not (np.isfinite(tint) and 0.0 <= tint <= 1.0):
        raise ValueError(f"{where}.{which}.tint must be a number in [0, 1], got {tint!r}")
    return {"angstrom": angstrom, "tint": float(tint)}


def check_haze_field(field: torch.Tensor, N: int, crop, who: str = "batch_nhhaze_from_windows") -> None:
    """the rows {seed, oy, ox, K, s, f0} of a CPU float64 [N,6] tensor against what the kernel takes for granted; ValueError names
    the row"""
    if not isinstance(field, torch.Tensor) or field.is_cuda or field.dtype != torch.float64 or tuple(field.shape) != (N, 6):
        raise TypeError(f"{who}: field must be a float64 [{N},6] tensor on the CPU")
    CH, CW = crop
    a = field.numpy()
    with np.errstate(all="ignore"):                 # every step calls this: all rows at once, the loop below only names a bad one
        seed, oy, ox, K, s, f0 = a.T
        fine = f0 * 2.0 ** (K - 1)
        whole = a[:, :4] == np.floor(a[:, :4])
        ok = (np.isfinite(a).all() and whole.all() and (seed >= 0).all() and (seed < 2 ** 32).all() and (oy >= 0).all()
              and (ox >= 0).all() and (K >= 1).all() and (K <= NH_MAX_OCTAVES).all() and (s >= 0).all() and (s < 1).all()
              and (f0 > 0).all() and (fine <= 0.5).all() and ((oy + CH) * fine < 2.0 ** 31).all()
              and ((ox + CW) * fine < 2.0 ** 31).all())
    if ok:
        return
    for n, (seed, oy, ox, K, s, f0) in enumerate(field.tolist()):
        def bad(what):
            return ValueError(f"{who}: field row {n}: {what}: {[seed, oy, ox, K, s, f0]}")
        if not (np.isfinite(seed) and seed == int(seed) and 0 <= seed < 2 ** 32):
            raise bad("seed must be an integer in [0, 2^32)")
        for name, o in (("oy", oy), ("ox", ox)):
            if not (np.isfinite(o) and o == int(o) and o >= 0):
                raise bad(f"{name} must be an integer >= 0")
        if not (np.isfinite(K) and K == int(K) and 1 <= K <= NH_MAX_OCTAVES):
            raise bad(f"K must be an integer in 1..{NH_MAX_OCTAVES}")
        if not 0.0 <= s < 1.0:
            raise bad("s must satisfy 0 <= s < 1")
        if not (np.isfinite(f0) and f0 > 0.0):
            raise bad("f0 must be finite and positive")
        fine = f0 * 2.0 ** (int(K) - 1)
        if fine > 0.5:
            raise bad(f"f0 * 2^(K-1) = {fine} > 0.5 (the finest cell is under 2 pixels)")
        if (oy + CH) * fine >= 2.0 ** 31 or (ox + CW) * fine >= 2.0 ** 31:
            raise bad("(origin + crop) * f0 * 2^(K-1) must stay below 2^31")


def batch_nhhaze_from_windows(clear: torch.Tensor, depth: Optional[torch.Tensor], geom: torch.Tensor, fog6: torch.Tensor,
                              field: torch.Tensor, crop, params: Optional[torch.Tensor] = None,
                              depth_range=DEFAULT_DEPTH_RANGE) -> torch.Tensor:
    """`batch_haze_from_windows` under patchy, wavelength-dependent haze (`adh_batch_nhhaze_from_u8`): `fog6` float32 [N,6] =
    {beta_r, beta_g, beta_b, A_r, A_g, A_b} and `field` (CPU float64 [N,6]) = {seed, oy, ox, K, s, f0}, both from `draw_nh_params`.
    Per source pixel the optical depth is scaled by m = 1 + s (2 f - 1), f in [0, 1] a K-octave value-noise field of coarsest
    frequency f0 (cells per pixel) anchored to the image: (oy, ox) is the window's origin in its image, so two crops of one image
    see the same cloud, and the field flips with the pixels.  t_c = exp(-beta_c m d), hazy_c = clamp(J_c t_c + A_c (1 - t_c)).
    The checks are `batch_haze_from_windows`' plus, before anything touches the device, `check_haze_field` (ValueError, naming
    the row): seed an integer in [0, 2^32), oy / ox integers >= 0, K an integer in 1..4, 0 <= s < 1, f0 finite and positive,
    f0 2^(K-1) <= 0.5, (origin + crop) f0 2^(K-1) < 2^31."""
    who = "batch_nhhaze_from_windows"
    if not isinstance(geom, torch.Tensor) or geom.is_cuda or geom.dtype != torch.int64 or geom.dim() != 2 or geom.shape[1] != 4:
        raise TypeError(f"{who}: geom must be an int64 [N,4] tensor on the CPU")
    if not isinstance(clear, torch.Tensor) or (depth is not None and not isinstance(depth, torch.Tensor)):
        raise TypeError(f"{who}: the caches must be tensors")
    CH, CW = _size2(crop)
    if CH < 1 or CW < 1:
        raise ValueError(f"{who}: crop must be at least 1 x 1, got {(CH, CW)}")
    N = geom.shape[0]
    if N < 1:
        raise ValueError(f"{who}: no windows")
    if not isinstance(fog6, torch.Tensor) or tuple(fog6.shape) != (N, 6):
        raise ValueError(f"{who}: fog6 must be a [{N},6] tensor of (beta_r, beta_g, beta_b, A_r, A_g, A_b)")
    check_haze_field(field, N, (CH, CW), who)
    if params is not None and tuple(params.shape) != (N, 5):
        raise ValueError(f"{who}: params must be [{N},5], got {tuple(params.shape)}")
    near, far = (float(v) for v in depth_range)
    if not (np.isfinite(near) and np.isfinite(far)):
        raise ValueError(f"{who}: depth_range must be finite, got {depth_range}")
    rows = geom.tolist()                                                                                    # Python ints: no wrap
    if depth is not None and any(do % 2 or dp % 2 or dp < CW * 2 for _, _, do, dp in rows):
        raise ValueError(f"{who}: depth offsets and pitches must be even and a pitch at least {CW * 2} bytes: {rows}")
    cbytes = clear.numel() * clear.element_size()
    if any(o < 0 or p < CW * 3 or o + (CH - 1) * p + CW * 3 > cbytes for o, p, _, _ in rows):
        raise IndexError(f"{who}: a {CH}x{CW} window leaves a clear cache of {cbytes} bytes: {rows}")
    dbytes = 0 if depth is None else depth.numel() * depth.element_size()
    if depth is not None and any(do < 0 or do + (CH - 1) * dp + CW * 2 > dbytes for _, _, do, dp in rows):
        raise IndexError(f"{who}: a {CH}x{CW} window leaves a depth cache of {dbytes} bytes: {rows}")
    for c, dt in ((clear, torch.uint8), (depth, torch.uint16)):
        if c is not None and (not c.is_cuda or c.dtype != dt or not c.is_contiguous() or c.device != clear.device):
            raise RuntimeError(f"adam-dehaze_amd: the cache must be a dense {dt} tensor on one cuda device, got {c.dtype} on "
                               f"{c.device} (no CPU fallback)")
    nblk = H.value("adh_batch_num_blocks", CH * CW)
    with torch.cuda.device(clear.device):
        gd = geom.contiguous().to(clear.device)
        fd = fog6.to(device=clear.device, dtype=torch.float32).contiguous()
        qd = field.contiguous().to(clear.device)
        pd = None if params is None else params.to(device=clear.device, dtype=torch.float32).contiguous()
        partial = None if pd is None else torch.empty(N * nblk, device=clear.device, dtype=torch.float64)
        out = torch.empty((N, 3, CH, CW), device=clear.device, dtype=torch.float32)
        H.call("adh_batch_nhhaze_from_u8", clear.data_ptr(), cbytes, H.ptr(depth), dbytes, gd.data_ptr(), fd.data_ptr(),
               qd.data_ptr(), near, far, H.ptr(pd), N, CH, CW, H.ptr(partial), nblk, out.data_ptr())
    return out


def draw_nh_params(n: int, rng, nonuniform: Optional[Dict], chromatic: Optional[Dict], sizes, origins, fog: torch.Tensor):
    """(fog6 float32 [n,6], field float64 [n,6]) for the n samples whose (beta, A) `fog` [n,2] `draw_haze_params` has drawn from
    `rng` before: these draws come after it, so a seed's (label, beta, A) do not depend on the settings.  `sizes` [n,2]: the cached
    images' (h, w) -- not the crop's; `origins` [n,2]: the windows' (y0, x0) in them (None: 0, 0).  Per sample, in order:
    nonuniform: s ~ U(amplitude), the coarsest cell ~ U(cell) as a fraction of min(h, w), f0 = 1 / (cell min(h, w)) as a float32
    value (capped at what keeps the finest cell 2 pixels wide), seed = rng.randint(0, 2**32), K = octaves; chromatic:
    alpha ~ U(angstrom), beta_c = beta (lambda_c / lambda_g)^-alpha with lambda = (610, 550, 465) nm and green keeping beta,
    A_c = clip(A + U(-tint, tint), 0, 1) in r, g, b order.  A setting that is None degenerates: s = 0 (K = 1, f0 = 0.5, seed 0),
    or beta_c = beta and A_c = A."""
    fog = torch.as_tensor(fog, dtype=torch.float32).reshape(n, 2).cpu()
    sizes = np.asarray(sizes, dtype=np.int64).reshape(n, 2)
    origins = np.zeros((n, 2), np.int64) if origins is None else np.asarray(origins, dtype=np.int64).reshape(n, 2)
    fog6, field = np.zeros((n, 6), np.float32), np.zeros((n, 6), np.float64)
    ratio = np.array(NH_WAVELENGTHS_NM, dtype=np.float64) / NH_WAVELENGTHS_NM[1]
    for i in range(n):
        beta, A = float(fog[i, 0]), float(fog[i, 1])
        s, K, f0, seed = 0.0, 1, 0.5, 0
        if nonuniform is not None:
            s = float(rng.uniform(*nonuniform["amplitude"]))
            cell = float(rng.uniform(*nonuniform["cell"]))
            K = int(nonuniform["octaves"])
            f0 = min(float(np.float32(1.0 / (cell * float(sizes[i].min())))), 0.5 / 2.0 ** (K - 1))
            seed = int(rng.randint(0, 2 ** 32))
        b3, A3 = np.full(3, beta), np.full(3, A)
        if chromatic is not None:
            alpha = float(rng.uniform(*chromatic["angstrom"]))
            b3 = beta * ratio ** (-alpha)
            b3[1] = beta
            A3 = np.clip(A + rng.uniform(-chromatic["tint"], chromatic["tint"], 3), 0.0, 1.0)
        fog6[i, :3], fog6[i, 3:] = b3, A3
        field[i] = (seed, origins[i, 0], origins[i, 1], K, s, f0)
    return torch.from_numpy(fog6), torch.from_numpy(field)


def _haze_dir(root: str, split: str) -> Optional[str]:
    """the directory that holds clear/ for `split`: <root>/<split>, else <root> itself, else None"""
    if not root:
        return None
    for d in (os.path.join(root, split), root):
        if os.path.isdir(os.path.join(d, "clear")):
            return d
    return None


def haze_index(root: str, split: str, depth: str = "folder") -> Optional[FolderIndex]:
    """The clear images of one split for haze synthesis, as records {clear, depth, name} sorted by name, or None when there is no
    `<root>/<split>/clear` and no `<root>/clear` directory.  Names must end in `.jpg` or `.png` (`folder_index`'s rule).  With
    `depth` 'folder' every record pairs with `depth/<stem>.png` beside `clear/`: a missing depth file raises FileNotFoundError
    and names it, a depth file whose size differs from its clear file's raises ValueError (both sizes come from the headers;
    nothing is decoded).  With 'radial' the records' `depth` is None and no depth folder is looked for."""
    if depth not in DEPTH_SOURCES:
        raise ValueError(f"dataset.synthetic_haze.depth must be one of {DEPTH_SOURCES}, got {depth!r}")
    d = _haze_dir(root, split)
    if d is None:
        return None
    from .image_io import image_size
    out = FolderIndex()
    out.split_dir = d
    for name in sorted(os.listdir(os.path.join(d, "clear"))):
        clear = os.path.join(d, "clear", name)
        if not name.endswith(IMAGE_SUFFIXES) or not os.path.isfile(clear):
            continue
        dpath = None
        if depth == "folder":
            dpath = os.path.join(d, "depth", os.path.splitext(name)[0] + ".png")
            if not os.path.isfile(dpath):
                raise FileNotFoundError(f"{clear} has no depth map: {dpath} does not exist (dataset.synthetic_haze.depth: radial "
                                        f"needs none)")
            try:
                cs, dsz = image_size(clear), image_size(dpath)
            except Exception as e:
                raise RuntimeError(f"cannot read the header of {clear} or {dpath}: {e}") from e
            if cs != dsz:
                raise ValueError(f"a depth map differs in size from its image: {dpath} is {dsz[0]}x{dsz[1]}, {clear} is "
                                 f"{cs[0]}x{cs[1]}")
        out.append({"clear": clear, "depth": dpath, "name": name})
    return out


class HazeSynthDataset:
    """One split of clear images (and their depth maps), resident on `device`, whose hazy role is rendered every step by
    `adh_batch_haze_from_u8`: `clear` uint8 and `depth` uint16 (None with `depth` 'radial'), for this rank's shard of the records
    of `haze_index` (samples rank, rank + world, ...).  The sibling of `FolderDataset`, with the same two layouts: dense at
    `img_size` ([L,H,W,3] and [L,H,W]; clear files through `adh_u8_resize_bilinear`, depth files through
    `adh_u16_resize_bilinear`), or with `crop_size` flat at the files' own sizes (`upscaled_size` where a crop does not fit), image
    k's pixels at byte `offsets[k]` and its depth at byte `depth_offsets[k]`, both multiples of 4.  The memory check counts 5 bytes
    per pixel, 3 without depth maps.  `depth_range` = (near, far): the scene depth of levels 0 and 65535.  `nonuniform` /
    `chromatic` (None: off; True: `NH_DEFAULTS`; or a mapping) render patchy / wavelength-dependent haze through
    `adh_batch_nhhaze_from_u8` instead; they change what is drawn per step, not what is cached."""

    def __init__(self, records: Sequence[Dict], img_size, device, rank: int = 0, world: int = 1, threads: int = 4,
                 split: str = "train", crop_size=None, depth: str = "folder", depth_range=DEFAULT_DEPTH_RANGE,
                 nonuniform=None, chromatic=None):
        from .image_io import image_size, load_depth, load_image
        self.nonuniform, self.chromatic = _nh_settings("nonuniform", nonuniform), _nh_settings("chromatic", chromatic)
        if depth not in DEPTH_SOURCES:
            raise ValueError(f"dataset.synthetic_haze.depth must be one of {DEPTH_SOURCES}, got {depth!r}")
        self.H, self.W = _size2(img_size)
        self.crop = None if crop_size is None else _size2(crop_size)
        self.device = torch.device(device)
        self.rank, self.world, self.total = rank, world, len(records)
        self.depth_source, self.depth_range = depth, (float(depth_range[0]), float(depth_range[1]))
        own = list(records[rank::world])
        self.names = [r["name"] for r in own]
        L = len(own)
        nthreads = max(1, min(int(threads), MAX_DECODE_THREADS))
        per_px = 5 if depth == "folder" else 3
        if self.crop is None:
            pixels, what, advice = L * self.H * self.W, f"{self.H}x{self.W}", "a smaller dataset.img_size"
            need = per_px * pixels
        else:
            def header(path):
                try:
                    return image_size(path)
                except Exception as e:
                    raise RuntimeError(f"cannot read image file {path}: {e}") from e
            with ThreadPoolExecutor(nthreads) as pool:
                own_sizes = list(pool.map(header, [r["clear"] for r in own]))
            sizes, offsets, doffsets, at, dat, upscaled = [], [], [], 0, 0, 0
            for hs in own_sizes:
                size = upscaled_size(hs[0], hs[1], self.crop)
                upscaled += size != tuple(hs)
                sizes.append(size)
                offsets.append(at)
                doffsets.append(dat)
                at += -(-size[0] * size[1] * 3 // 4) * 4             # every slot of either cache starts on a multiple of 4
                dat += -(-size[0] * size[1] * 2 // 4) * 4
            self.sizes = np.array(sizes, dtype=np.int64).reshape(-1, 2)
            self.offsets, self.depth_offsets = np.array(offsets, dtype=np.int64), np.array(doffsets, dtype=np.int64)
            self.cache_bytes, self.depth_bytes = at, dat
            need, advice = at + (dat if depth == "folder" else 0), "a smaller dataset"
            what = f"their own sizes ({upscaled} upscaled to hold a {self.crop[0]}x{self.crop[1]} crop)"
        if self.device.type != "cuda":
            raise RuntimeError(f"adam-dehaze_amd: the dataset cache lives on a cuda device, got {self.device} (no CPU fallback)")
        free = torch.cuda.mem_get_info(self.device)[0]
        if need > free // 2:
            raise RuntimeError(f"the {split} split needs {need} bytes of device memory as a cache of clear images"
                               f"{' and depth maps' if depth == 'folder' else ''} ({L} images at {what}, {per_px} bytes per "
                               f"pixel), more than half of the {free} bytes free on {self.device}; a streaming loader is not "
                               f"built: use {advice} or more ranks")
        if self.crop is None:
            self.clear = torch.empty((L, self.H, self.W, 3), dtype=torch.uint8, device=self.device)
            self.depth = torch.empty((L, self.H, self.W), dtype=torch.uint16, device=self.device) if depth == "folder" else None
        else:
            self.clear = torch.empty((self.cache_bytes,), dtype=torch.uint8, device=self.device)
            self.depth = torch.empty((self.depth_bytes // 2,), dtype=torch.uint16, device=self.device) if depth == "folder" else None

        def decode(job):
            try:
                return load_depth(job[2], raw=True) if job[0] == "depth" else load_image(job[2])
            except Exception as e:
                raise RuntimeError(f"cannot read image file {job[2]}: {e}") from e
        jobs = [(role, slot, r[role]) for slot, r in enumerate(own) for role in ("clear", "depth") if r.get(role) is not None
                and (role == "clear" or depth == "folder")]
        with ThreadPoolExecutor(nthreads) as pool, torch.cuda.device(self.device):
            for at in range(0, len(jobs), 4 * nthreads):        # a few files per thread in flight: decoded files do not pile up
                chunk = jobs[at:at + 4 * nthreads]
                for (role, slot, path), img in zip(chunk, pool.map(decode, chunk)):
                    h, w = img.shape[:2]
                    oh, ow = (self.H, self.W) if self.crop is None else self.sizes[slot].tolist()
                    src = img.contiguous().to(self.device)
                    if role == "clear":
                        at_byte = slot * oh * ow * 3 if self.crop is None else int(self.offsets[slot])
                        c = img.shape[2]
                        H.call("adh_u8_resize_bilinear", src.data_ptr(), w * c, h, w, c, self.clear.data_ptr() + at_byte, oh, ow)
                    else:
                        at_byte = slot * oh * ow * 2 if self.crop is None else int(self.depth_offsets[slot])
                        bpp = img.element_size()
                        H.call("adh_u16_resize_bilinear", src.data_ptr(), w * bpp, h, w, bpp, self.depth.data_ptr() + at_byte, oh, ow)
        print(f"Loaded {self.total} clear images for {split} split (haze synthesized on the device, depth: {depth})")
        print(f"  device cache: {L} images at {what} on {self.device}, {need / 2 ** 20:.1f} MiB ({need} bytes)"
              + (f" (rank {rank} of {world})" if world > 1 else ""))

    def __len__(self):
        return len(self.names)

    def geometry(self, index: np.ndarray, origins: Optional[np.ndarray] = None) -> torch.Tensor:
        """int64 [n,4] rows of `batch_haze_from_windows` for the shard's images `index`: dense mode {i*H*W*3, W*3, i*H*W*2, W*2},
        crop mode the windows at `origins` [n,2] (y0, x0)"""
        index = np.asarray(index, dtype=np.int64)
        if self.crop is None:
            px = self.H * self.W
            g = np.stack([index * px * 3, np.full_like(index, self.W * 3), index * px * 2, np.full_like(index, self.W * 2)], axis=1)
        else:
            sizes, origins = self.sizes[index], np.asarray(origins, dtype=np.int64)
            at = origins[:, 0] * sizes[:, 1] + origins[:, 1]
            g = np.stack([self.offsets[index] + at * 3, sizes[:, 1] * 3, self.depth_offsets[index] + at * 2, sizes[:, 1] * 2], axis=1)
        return torch.from_numpy(np.ascontiguousarray(g, dtype=np.int64))

    def epoch(self, epoch: int, batch_size: int, seed: int, train: bool, augment: bool = True) -> Iterator[Dict]:
        """The batch dicts of `FolderDataset.epoch` plus 'beta' and 'airlight' (float32 [n], device), in the order of `epoch_plan`;
        'intensity' is the drawn density label.  train: from this loader's RandomState(seed + 1000 * rank + epoch), per batch, the
        augment rows (when `augment`), the crop origins (crop mode), then `draw_haze_params`: every epoch re-renders every image
        under fresh haze.  Otherwise: the centre crop, no rows, and `fixed_haze_params(seed, sample numbers)`, the same in every
        epoch and for every world size.  The clear role comes from `batch_from_cache` / `batch_from_windows` with the same rows.
        With `nonuniform` or `chromatic`: `draw_nh_params` draws after `draw_haze_params` (train: from the loader's stream, for the
        batch; otherwise per sample from its own RandomState, `fixed_nh_params`), the field's origin is the crop origin, and the
        dict gains 'beta_rgb', 'airlight_rgb' (float32 [n,3], device) and 'haze_field' (float64 [n,6], CPU); 'beta' and
        'airlight' stay the drawn ones."""
        if self.total == 0 or (not train and len(self) == 0):
            return
        rng = np.random.RandomState(seed + 1000 * self.rank + epoch)
        for samples in epoch_plan(self.total, self.world, self.rank, batch_size, seed, epoch, train):
            index = torch.from_numpy((samples - self.rank) // self.world)
            params = draw_augment_params(index.numel(), rng) if train and augment else None
            origins = None
            if self.crop is not None:
                sizes = self.sizes[index.numpy()]
                origins = draw_crop_origins(sizes, self.crop, rng) if train else centre_origins(sizes, self.crop)
            nh = self.nonuniform is not None or self.chromatic is not None
            geom = self.geometry(index.numpy(), origins)
            if nh:
                n = index.numel()
                sizes = self.sizes[index.numpy()] if self.crop is not None else np.tile([self.H, self.W], (n, 1))
                if train:
                    labels, fog = draw_haze_params(n, rng)
                    fog6, field = draw_nh_params(n, rng, self.nonuniform, self.chromatic, sizes, origins, fog)
                else:
                    labels, fog, fog6, field = fixed_nh_params(seed, samples, self.nonuniform, self.chromatic, sizes, origins)
                fog, fog6 = fog.to(self.device), fog6.to(self.device)
                hazy = batch_nhhaze_from_windows(self.clear, self.depth, geom, fog6, field, self.crop or (self.H, self.W), params,
                                                 self.depth_range)
            else:
                labels, fog = draw_haze_params(index.numel(), rng) if train else fixed_haze_params(seed, samples)
                fog = fog.to(self.device)
                hazy = batch_haze_from_windows(self.clear, self.depth, geom, fog, self.crop or (self.H, self.W), params,
                                               self.depth_range)
            if self.crop is None:
                clear = batch_from_cache(self.clear, index, params)
            else:
                clear = batch_from_windows(self.clear, geom[:, :2].contiguous(), self.crop, params)
            batch = {"hazy": hazy, "clear": clear, "intensity": labels.to(self.device), "beta": fog[:, 0].contiguous(),
                     "airlight": fog[:, 1].contiguous(), "name": [self.names[i] for i in index.tolist()]}
            if nh:
                batch.update(beta_rgb=fog6[:, :3].contiguous(), airlight_rgb=fog6[:, 3:].contiguous(), haze_field=field)
            yield batch


def synthesize_tree(input_dir: str, output_dir: str, depth_dir: Optional[str] = None, seed: int = 0, device="cuda",
                    depth_range=DEFAULT_DEPTH_RANGE, nonuniform=None, chromatic=None) -> List[Dict]:
    """`main.py --mode synthesize`: every `.jpg` / `.png` file of `input_dir` (sorted) rendered once per density level at its own
    size, as `<output_dir>/{low,medium,high}/{hazy,clear}/<stem>.png` -- the layout `folder_index` reads -- plus
    `<output_dir>/synthesize.json` with each file's beta and A.  The hazy bytes are `image_io.image_to_u8` of what
    `batch_haze_from_windows` gives for the whole image (no rows), i.e. what training with `dataset.synthetic_haze` sees for that
    (beta, A); the clear file holds the cached RGB bytes.  `depth_dir`: `<stem>.png` per clear file (a missing or differently
    sized one raises); None: the reference's radial depth map.  Per file, in order, from RandomState(seed): (beta, A) of low, of
    medium, of high (`draw_fog_params`).  `nonuniform` / `chromatic` (None: off; True: `NH_DEFAULTS`; or a mapping, checked before
    a file is read): the three levels are rendered by `batch_nhhaze_from_windows` with what `draw_nh_params` draws from the same
    stream after the file's (beta, A), origin (0, 0), and every record gains `beta_rgb`, `airlight_rgb` and `haze_field`
    ({seed, oy, ox, K, s, f0}); without either the files and the json are what they were.  Returns the records written to the
    json."""
    import json
    from .image_io import image_size, image_to_u8, load_depth, load_image, save_image
    device = torch.device(device)
    nonuniform, chromatic = _nh_settings("nonuniform", nonuniform, "synthesize"), _nh_settings("chromatic", chromatic, "synthesize")
    nh = nonuniform is not None or chromatic is not None
    if device.type != "cuda":
        raise RuntimeError(f"adam-dehaze_amd: haze is synthesized on a cuda device, got {device} (no CPU fallback)")
    if not os.path.isdir(input_dir):
        raise ValueError(f"--input {input_dir}: not a directory of clear images")
    names = [n for n in sorted(os.listdir(input_dir)) if n.endswith(IMAGE_SUFFIXES) and os.path.isfile(os.path.join(input_dir, n))]
    if not names:
        raise ValueError(f"--input {input_dir}: no .jpg or .png file")
    stems = [os.path.splitext(n)[0] for n in names]
    twice = sorted({s for s in stems if stems.count(s) > 1})
    if twice:
        raise ValueError(f"input files share a base name and would overwrite each other's output: {', '.join(twice)}")
    for level in LEVEL_NAMES:
        for role in ("hazy", "clear"):
            os.makedirs(os.path.join(output_dir, level, role), exist_ok=True)
    rng = np.random.RandomState(seed)
    records = []
    with torch.cuda.device(device):
        for name, stem in zip(names, stems):
            path = os.path.join(input_dir, name)
            img = load_image(path)
            h, w, c = img.shape
            clear = torch.empty((h * w * 3 + 3) // 4 * 4, dtype=torch.uint8, device=device)
            H.call("adh_u8_resize_bilinear", img.contiguous().to(device).data_ptr(), w * c, h, w, c, clear.data_ptr(), h, w)
            depth, dpath = None, None
            if depth_dir is not None:
                dpath = os.path.join(depth_dir, stem + ".png")
                if not os.path.isfile(dpath):
                    raise FileNotFoundError(f"{path} has no depth map: {dpath} does not exist")
                if image_size(dpath) != (h, w):
                    raise ValueError(f"a depth map differs in size from its image: {dpath} is {image_size(dpath)}, {path} is {(h, w)}")
                d = load_depth(dpath, raw=True)
                depth = torch.empty((h * w + 1) // 2 * 2, dtype=torch.uint16, device=device)
                H.call("adh_u16_resize_bilinear", d.contiguous().to(device).data_ptr(), w * d.element_size(), h, w, d.element_size(),
                       depth.data_ptr(), h, w)
            beta, A = draw_fog_params(LEVEL_NAMES, rng)
            fog = torch.stack([beta, A], dim=1).to(torch.float32)
            geom = torch.tensor([[0, w * 3, 0, w * 2]] * len(LEVEL_NAMES), dtype=torch.int64)
            if nh:
                fog6, field = draw_nh_params(len(LEVEL_NAMES), rng, nonuniform, chromatic, [(h, w)] * len(LEVEL_NAMES), None, fog)
                hazy = image_to_u8(batch_nhhaze_from_windows(clear, depth, geom, fog6, field, (h, w), None, depth_range)).cpu()
            else:
                hazy = image_to_u8(batch_haze_from_windows(clear, depth, geom, fog, (h, w), None, depth_range)).cpu()
            clear_host = clear[:h * w * 3].reshape(h, w, 3).cpu()
            for k, level in enumerate(LEVEL_NAMES):
                save_image(os.path.join(output_dir, level, "hazy", stem + ".png"), hazy[k])
                save_image(os.path.join(output_dir, level, "clear", stem + ".png"), clear_host)
                records.append({"file": path, "depth": dpath, "level": level, "name": stem + ".png", "height": h, "width": w,
                                "beta": float(fog[k, 0]), "airlight": float(fog[k, 1])})
                if nh:
                    records[-1].update(beta_rgb=[float(v) for v in fog6[k, :3]], airlight_rgb=[float(v) for v in fog6[k, 3:]],
                                       haze_field=[float(v) for v in field[k]])
    head = {"seed": int(seed), "depth_range": [float(v) for v in depth_range]}
    if nh:
        head.update(nonuniform=nonuniform, chromatic=chromatic)
    with open(os.path.join(output_dir, "synthesize.json"), "w") as f:
        json.dump({**head, "files": records}, f, indent=2)
    print(f"synthesized {len(names)} clear files at 3 levels into {output_dir}")
    return records


def _haze_loader(config, ds, settings, split: str, device, rank: Optional[int], world: Optional[int]) -> Callable:
    """`folder_loader` for `dataset.synthetic_haze` = `settings`"""
    unknown = sorted(set(settings) - {"depth", "depth_range", "nonuniform", "chromatic"})
    if unknown:
        raise ValueError(f"dataset.synthetic_haze: unknown keys {unknown} (known: depth, depth_range, nonuniform, chromatic)")
    nonuniform = _nh_settings("nonuniform", settings.get("nonuniform"))
    chromatic = _nh_settings("chromatic", settings.get("chromatic"))
    depth = settings.get("depth", "folder")
    if depth not in DEPTH_SOURCES:
        raise ValueError(f"dataset.synthetic_haze.depth must be one of {DEPTH_SOURCES}, got {depth!r}")
    rng_ = settings.get("depth_range", list(DEFAULT_DEPTH_RANGE))
    if not isinstance(rng_, (list, tuple)) or len(rng_) != 2:
        raise ValueError(f"dataset.synthetic_haze.depth_range must be [near, far], got {rng_!r}")
    depth_range = (float(rng_[0]), float(rng_[1]))
    root = ds.get({"train": "train_path", "val": "val_path"}.get(split, "test_path"))
    split_dir = _haze_dir(root, split)
    if split_dir is None:
        raise RuntimeError(f"dataset.synthetic_haze is configured but the {split} split has no clear/ folder under {root!r} (looked "
                           f"for <root>/{split}/clear and <root>/clear); noise frames are not substituted")
    rank = int(os.environ.get("RANK", "0")) if rank is None else rank
    world = int(os.environ.get("WORLD_SIZE", "1")) if world is None else world
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    crop = ds.get("crop_size")
    crop = None if crop is None else _size2(crop)
    key = ("synthetic_haze", os.path.realpath(split_dir), split, _size2(ds["img_size"]), str(device), rank, world, crop, depth,
           depth_range)
    if key not in _CACHES:
        records = haze_index(root, split, depth)
        if not records:
            raise RuntimeError(f"{split_dir}/clear: the {split} split has no .jpg or .png file")
        _CACHES[key] = HazeSynthDataset(records, ds["img_size"], device, rank, world, threads=int(ds.get("num_workers", 4)),
                                        split=split, crop_size=crop, depth=depth, depth_range=depth_range)
    cache = _CACHES[key]
    if (nonuniform, chromatic) != (cache.nonuniform, cache.chromatic):
        cache = copy.copy(cache)        # the caches are shared (the settings change no cached byte); the draws are this loader's
        cache.nonuniform, cache.chromatic = nonuniform, chromatic
    batch_size, seed, train = int(ds["batch_size"]), int(config.get("seed", 0)), split == "train"
    augment = bool(ds.get("augmentation", True))

    def epochs(epoch=0):
        return cache.epoch(epoch, batch_size, seed, train, augment)
    epochs.dataset = cache          # the resident cache, for a caller that wants to look at what is served
    return epochs


_CACHES: Dict[tuple, object] = {}     # (resolved split directory, split, (h, w), device, rank, world, crop) -> the built cache


def folder_loader(config, split: str, device, rank: Optional[int] = None, world: Optional[int] = None) -> Optional[Callable]:
    """`epoch -> iterable of batch dicts` over the image folders of `split` ('train' | 'val' | 'test'), or None when
    `folder_index` finds none under `dataset.train_path` / `val_path` / `test_path` (data/dataset.py:233-241).  rank / world
    default to the process's RANK / WORLD_SIZE.  The cache of a split is built once per process and kept, so the stages of
    train_all and the evaluators share it.  `dataset.num_workers` is the number of decode threads.  `dataset.crop_size` (int or
    [h, w]; absent or null: off) caches every pair at its own resolution and serves random crops of that size to training and
    centre crops to validation and test (`FolderDataset`); the synthetic fallback does not read it and keeps using `img_size`.
    `dataset.synthetic_haze` (a mapping; absent: off) trains from clear images instead: `<root>/<split>/clear/<name>` (else
    `<root>/clear/<name>`) with `depth/<stem>.png` beside it, the hazy role rendered on the device every step
    (`HazeSynthDataset`).  Keys: `depth: folder | radial` (default folder) and `depth_range: [near, far]` (default [0.3, 1.0]); both
    join the cache key.  `nonuniform: {amplitude: [lo, hi], cell: [lo, hi], octaves: K}` (patchy haze: the optical depth scaled by
    1 + s (2 f - 1), s ~ U(amplitude), f a K-octave noise field whose coarsest cell is ~ U(cell) of the image's shorter side;
    defaults [0.2, 0.8], [0.15, 0.5], 3) and `chromatic: {angstrom: [lo, hi], tint: x}` (beta_c = beta (lambda_c / 550 nm)^-alpha,
    A_c = A + U(-x, x); defaults [0.0, 1.3], 0.05) switch the renderer to `adh_batch_nhhaze_from_u8`; an empty mapping takes the
    defaults; they change no cached byte and do not join the cache key.  A configured `synthetic_haze` whose split has no
    `clear/` folder raises."""
    ds = config.get("dataset", {})
    if isinstance(ds.get("synthetic_haze"), Mapping):
        return _haze_loader(config, ds, ds["synthetic_haze"], split, device, rank, world)
    root = ds.get({"train": "train_path", "val": "val_path"}.get(split, "test_path"))
    split_dir = _split_dir(root, split)
    if split_dir is None:
        return None
    rank = int(os.environ.get("RANK", "0")) if rank is None else rank
    world = int(os.environ.get("WORLD_SIZE", "1")) if world is None else world
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    crop = ds.get("crop_size")
    crop = None if crop is None else _size2(crop)
    key = (os.path.realpath(split_dir), split, _size2(ds["img_size"]), str(device), rank, world, crop)
    if key not in _CACHES:
        records = folder_index(root, split)
        if not records:
            raise RuntimeError(f"{records.split_dir}: the {split} split has image folders but no hazy / clear pair "
                               f"({records.skipped} hazy files without a clear file)")
        _CACHES[key] = FolderDataset(records, ds["img_size"], device, rank, world, threads=int(ds.get("num_workers", 4)),
                                     split=split, crop_size=crop)
    cache = _CACHES[key]
    batch_size, seed, train = int(ds["batch_size"]), int(config.get("seed", 0)), split == "train"
    augment = bool(ds.get("augmentation", True))
    return lambda epoch=0: cache.epoch(epoch, batch_size, seed, train, augment)
