"""The host side of crop training (data.draw_crop_origins, centre_origins, upscaled_size, crop_windows, the host checks of
batch_from_windows and the draw order of FolderDataset.epoch), without a GPU."""
import numpy as np
import pytest
import torch

from adam_dehaze_amd import data as D


class _Recording:
    """a RandomState that notes every randint call"""

    def __init__(self, seed):
        self.rng, self.calls = np.random.RandomState(seed), []

    def randint(self, *a, **k):
        self.calls.append(a)
        return self.rng.randint(*a, **k)


def test_draw_crop_origins():
    sizes = np.array([[40, 56], [32, 32], [24, 100], [57, 24]], np.int64)
    rec = _Recording(5)
    got = D.draw_crop_origins(sizes, (24, 24), rec)
    assert got.dtype == np.int64 and got.shape == (4, 2)
    assert rec.calls == [(0, 17), (0, 33), (0, 9), (0, 9), (0, 1), (0, 77), (0, 34), (0, 1)]      # y then x, sample after sample
    plain = np.random.RandomState(5)
    assert got.tolist() == [[plain.randint(0, h - 23), plain.randint(0, w - 23)] for h, w in sizes.tolist()]
    assert (got >= 0).all() and (got + 24 <= sizes).all()
    assert np.array_equal(D.draw_crop_origins(sizes, 24, np.random.RandomState(5)), got)          # reproducible; int = square
    many = np.concatenate([D.draw_crop_origins(sizes, (24, 20), np.random.RandomState(s)) for s in range(200)])
    big = np.tile(sizes, (200, 1))
    assert (many >= 0).all() and (many + [24, 20] <= big).all()
    assert many[0::4, 0].max() == 16 and many[0::4, 0].min() == 0 and many[3::4, 1].max() == 4    # both ends are reached
    assert D.draw_crop_origins(np.zeros((0, 2), np.int64), 24, rec).shape == (0, 2)


def test_centre_origins():
    sizes = np.array([[40, 56], [32, 32], [24, 25], [24, 24]], np.int64)
    got = D.centre_origins(sizes, (24, 24))
    assert got.dtype == np.int64 and got.tolist() == [[8, 16], [4, 4], [0, 0], [0, 0]]
    assert D.centre_origins(sizes, (20, 24)).tolist() == [[10, 16], [6, 4], [2, 0], [2, 0]]


def test_upscaled_size():
    assert D.upscaled_size(32, 32, (36, 44)) == (44, 44)              # the width binds: 32 -> 44, the height follows
    assert D.upscaled_size(40, 56, (36, 44)) == (40, 56)              # the crop fits: unchanged
    assert D.upscaled_size(36, 44, (36, 44)) == (36, 44)              # exactly the crop
    assert D.upscaled_size(20, 100, (36, 44)) == (36, 180)            # height-limited: 20 -> 36, 100 * 36 / 20 = 180
    assert D.upscaled_size(30, 50, (36, 44)) == (36, 60)
    assert D.upscaled_size(100, 40, (36, 44)) == (110, 44)            # one side fits, the other does not
    assert D.upscaled_size(7, 9, (36, 44)) == (36, 46)                # 9 * 36 / 7 = 46.29
    assert D.upscaled_size(9, 7, (36, 44)) == (57, 44)                # 9 * 44 / 7 = 56.57, half up
    assert D.upscaled_size(3, 2, (4, 4)) == (6, 4) and D.upscaled_size(2, 3, (5, 5)) == (5, 8)    # 7.5 rounds up
    assert D.upscaled_size(32, 32, 24) == (32, 32)
    for h, w in [(1, 1), (5, 300), (300, 5), (35, 43), (36, 43), (35, 44)]:
        oh, ow = D.upscaled_size(h, w, (36, 44))
        assert oh >= 36 and ow >= 44 and (oh == 36 or ow == 44)       # holds one crop, and is the smallest that does


def test_crop_windows():
    offsets, sizes = np.array([0, 6720, 9792]), np.array([[40, 56], [32, 32], [24, 25]])
    origins = np.array([[8, 16], [0, 0], [0, 1]])
    w = D.crop_windows(offsets, sizes, origins)
    assert w.dtype == torch.int64 and w.tolist() == [[(8 * 56 + 16) * 3, 168], [6720, 96], [9792 + 3, 75]]


def test_windows_are_checked_on_the_host_before_any_device():
    cache = torch.zeros(40 * 56 * 3 + 4, dtype=torch.uint8)           # a CPU tensor: a passing check fails on the device test
    good = torch.tensor([[0, 168], [(16 * 56 + 32) * 3, 168]], dtype=torch.int64)        # the second ends with the image
    for bad in ([[-1, 168]], [[0, 71]], [[(16 * 56 + 32) * 3 + 5, 168]], [[0, 168], [(17 * 56) * 3, 168]], [[0, 400]],
                [[2 ** 62, 168]], [[0, 2 ** 62]]):
        with pytest.raises(IndexError):
            D.batch_from_windows(cache, torch.tensor(bad, dtype=torch.int64), (24, 24))
    for bad in (good.to(torch.int32), good.tolist(), good[0], good.reshape(1, 4)):
        with pytest.raises(TypeError):
            D.batch_from_windows(cache, bad, (24, 24))
    with pytest.raises(ValueError):
        D.batch_from_windows(cache, good, (24, 24), params=torch.zeros(3, 5))
    with pytest.raises(ValueError):
        D.batch_from_windows(cache, good, (24, 24), params=torch.zeros(2, 4))
    with pytest.raises(ValueError):
        D.batch_from_windows((cache, cache[:-4]), good, (24, 24))                          # caches of two lengths
    with pytest.raises(ValueError):
        D.batch_from_windows(cache.reshape(-1, 4), good, (24, 24))                         # not flat
    with pytest.raises(ValueError):
        D.batch_from_windows(cache, good[:0], (24, 24))
    with pytest.raises(ValueError):
        D.batch_from_windows(cache, good, (0, 24))
    with pytest.raises(RuntimeError, match="cuda"):                   # all in range: the next check is the device's
        D.batch_from_windows(cache, good, (24, 24), params=torch.zeros(2, 5))
    with pytest.raises(RuntimeError, match="cuda"):
        D.batch_from_windows((cache, cache.clone()), torch.tensor([[4, 72]], dtype=torch.int64), (1, 24))


def test_the_lpips_term_can_be_switched_off_for_small_crops():
    from adam_dehaze_amd import loss as Ls
    for cfg in (None, {}, {"loss": None}, {"loss": {"lambda_ssim": 0.2}}, {"loss": {"perceptual": True}}):
        assert Ls._perceptual(cfg) == {}                              # the loss is built exactly as before
    assert Ls._perceptual({"loss": {"perceptual": False}}) == {"perceptual": False}
    assert Ls.DehazingLoss(content=False, **Ls._perceptual({"loss": {"perceptual": False}})).perceptual_loss is None


def _host_dataset(crop, sizes, rank=0, world=1):
    """a FolderDataset as its constructor leaves it, without the device cache"""
    ds = object.__new__(D.FolderDataset)
    L = len(sizes)
    ds.H = ds.W = 16
    ds.crop, ds.device, ds.rank, ds.world, ds.total = crop, torch.device("cpu"), rank, world, L * world
    ds.names = [f"f{k}" for k in range(L)]
    ds.labels = torch.arange(L) % 3
    ds.hazy = ds.clear = torch.zeros(1, dtype=torch.uint8)
    if crop is not None:
        ds.sizes = np.array(sizes, np.int64)
        ds.offsets = np.cumsum([0] + [-(-h * w * 3 // 4) * 4 for h, w in sizes[:-1]]).astype(np.int64)
    return ds


def test_without_crop_size_epoch_draws_what_it_drew(monkeypatch):
    ds = _host_dataset(None, [(16, 16)] * 7, rank=1, world=2)
    seen = []
    monkeypatch.setattr(D, "batch_from_cache", lambda caches, index, params: seen.append((index, params)) or ("h", "c"))
    monkeypatch.setattr(D, "draw_crop_origins", lambda *a, **k: pytest.fail("no origin may be drawn"))
    monkeypatch.setattr(D, "batch_from_windows", lambda *a, **k: pytest.fail("no window may be served"))
    batches = list(ds.epoch(3, 4, 42, train=True))
    assert [b["hazy"] for b in batches] == ["h", "h"] and set(batches[0]) == {"hazy", "clear", "intensity", "name"}
    rng = np.random.RandomState(42 + 1000 * 1 + 3)
    plan = D.epoch_plan(14, 2, 1, 4, 42, 3, True)
    assert len(seen) == len(plan) == 2
    for (index, params), samples in zip(seen, plan):
        assert index.tolist() == ((samples - 1) // 2).tolist()
        assert torch.equal(params, D.draw_augment_params(len(samples), rng))
    rest = rng.randint(2147483647)
    tail = np.random.RandomState(42 + 1000 * 1 + 3)
    for samples in plan:
        D.draw_augment_params(len(samples), tail)
    assert rest == tail.randint(2147483647)
    seen.clear()
    n = len(list(ds.epoch(0, 4, 42, train=True, augment=False))) + len(list(ds.epoch(0, 4, 42, train=False)))
    assert n == len(seen) == 4 and all(p is None for _, p in seen)


def test_crop_epoch_draws_rows_then_origins(monkeypatch):
    sizes = [(40, 56), (32, 32), (24, 24), (30, 77), (25, 24)]
    ds = _host_dataset((24, 24), sizes)
    seen = []
    monkeypatch.setattr(D, "batch_from_windows", lambda caches, w, crop, params: seen.append((w, crop, params)) or ("h", "c"))
    monkeypatch.setattr(D, "batch_from_cache", lambda *a, **k: pytest.fail("the dense gather may not run"))
    names = [b["name"] for b in ds.epoch(2, 2, 7, train=True)]
    rng = np.random.RandomState(7 + 2)
    plan = D.epoch_plan(5, 1, 0, 2, 7, 2, True)
    assert names == [[f"f{i}" for i in s] for s in plan] and len(seen) == 3
    for (w, crop, params), s in zip(seen, plan):
        assert crop == (24, 24)
        assert torch.equal(params, D.draw_augment_params(len(s), rng))                     # the rows first,
        origins = D.draw_crop_origins(ds.sizes[s], (24, 24), rng)                          # then the origins
        assert torch.equal(w, D.crop_windows(ds.offsets[s], ds.sizes[s], origins))
    seen.clear()
    list(ds.epoch(2, 2, 7, train=True, augment=False))
    rng = np.random.RandomState(7 + 2)
    for (w, crop, params), s in zip(seen, plan):                      # without rows the origins are the first draws
        assert params is None
        assert torch.equal(w, D.crop_windows(ds.offsets[s], ds.sizes[s], D.draw_crop_origins(ds.sizes[s], (24, 24), rng)))
    seen.clear()
    list(ds.epoch(5, 2, 7, train=False))
    for (w, crop, params), s in zip(seen, D.epoch_plan(5, 1, 0, 2, 7, 5, False)):
        assert params is None
        assert torch.equal(w, D.crop_windows(ds.offsets[s], ds.sizes[s], D.centre_origins(ds.sizes[s], (24, 24))))
