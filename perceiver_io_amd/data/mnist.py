"""MNIST data module (reference ``data/mnist.py:1-55``, SURVEY #28).

Reads the standard IDX files (``train-images-idx3-ubyte[.gz]`` …) from ``<data_dir>/MNIST/raw``
or ``<data_dir>``; no download (offline).  ``synthetic=True`` (or ``synthetic='auto'`` with the
files absent) generates class-structured 28×28 images.  Transforms as the reference:
[RandomCrop], scale to [0, 1], Normalize(0.5, 0.5), channels-last.  The train split holds
out ``val_split`` images for validation (pl_bolts semantics), the test split is MNIST test.
Defect D7 fixed: ``image_shape`` reflects ``random_crop``.

``device_augment=True`` moves the transforms to the device: the datasets yield the raw uint8 image
and the label, the module's ``augment`` (:class:`~perceiver_io_amd.data.augment.DeviceAugment`)
draws the crop offsets / flips per batch and ``ops.batch_augment`` crops, flips and normalizes
there (bit for bit the host transform for the same offsets).  ``NpyImageDataModule`` trains on a
pre-decoded uint8 ``.npy`` dataset through the same path.
"""
from __future__ import annotations

import gzip
import os
import struct
from typing import Optional, Union

import torch

from .augment import DeviceAugment, RandAugment
from .registry import register_datamodule
from .synthetic import SyntheticImages


def _read_idx(path: str) -> torch.Tensor:
    op = gzip.open if path.endswith(".gz") else open
    with op(path, "rb") as f:
        data = f.read()
    magic = struct.unpack(">I", data[:4])[0]
    nd = magic & 0xFF
    dims = struct.unpack(">" + "I" * nd, data[4:4 + 4 * nd])
    return torch.frombuffer(bytearray(data[4 + 4 * nd:]), dtype=torch.uint8).reshape(dims)


def _find(root: str, stem: str) -> Optional[str]:
    for d in (os.path.join(root, "MNIST", "raw"), root):
        for ext in ("", ".gz"):
            p = os.path.join(d, stem + ext)
            if os.path.exists(p):
                return p
    return None


class _Transformed(torch.utils.data.Dataset):
    def __init__(self, images: torch.Tensor, labels: torch.Tensor, crop: Optional[int], normalize: bool,
                 channels_last: bool, train: bool):
        self.images, self.labels = images, labels
        self.crop, self.normalize, self.cl, self.train = crop, normalize, channels_last, train

    def __len__(self):
        return len(self.labels)

    def __getitem__(self, i):
        x = self.images[i].float() / 255.0  # (H, W)
        if self.crop:
            h, w = x.shape
            if self.train:
                top = int(torch.randint(0, h - self.crop + 1, (1,)))
                left = int(torch.randint(0, w - self.crop + 1, (1,)))
            else:
                top, left = (h - self.crop) // 2, (w - self.crop) // 2
            x = x[top:top + self.crop, left:left + self.crop]
        if self.normalize:
            x = (x - 0.5) / 0.5
        x = x.unsqueeze(-1) if self.cl else x.unsqueeze(0)
        return x, int(self.labels[i])


class _RawImages(torch.utils.data.Dataset):
    """Raw ``(H, W, C)`` uint8 images and labels: the device-augmentation path (no transform here)."""

    def __init__(self, images, labels):
        self.images, self.labels = images, labels

    def __len__(self):
        return len(self.labels)

    def __getitem__(self, i):
        x = self.images[i]
        if not torch.is_tensor(x):  # a row of a memory-mapped array
            import numpy as np

            x = torch.from_numpy(np.array(x))
        return (x.unsqueeze(-1) if x.dim() == 2 else x), int(self.labels[i])


def _rand_augment(hparams: dict, device_augment: bool, source_hw, ops: int, magnitude: int, fill: int):
    """The ``RandAugment`` of a data module's ``rand_augment_*`` options (None when unset), which are
    recorded in ``hparams`` only when set."""
    if int(ops) <= 0:
        return None
    if not device_augment:
        raise ValueError("rand_augment_ops > 0 needs device_augment=true (RandAugment runs on the raw uint8 batch "
                         "on the device)")
    hparams.update(rand_augment_ops=int(ops), rand_augment_magnitude=int(magnitude), rand_augment_fill=int(fill))
    return RandAugment(source_hw, num_ops=int(ops), magnitude=int(magnitude), fill=int(fill))


@register_datamodule
class MNISTDataModule:
    name = "mnist"

    def __init__(self, channels_last: bool = True, random_crop: Optional[int] = None, data_dir: Optional[str] = ".cache",
                 val_split: Union[int, float] = 10000, num_workers: int = 3, normalize: bool = True, pin_memory: bool = False,
                 batch_size: int = 32, seed: int = 42, shuffle: bool = True, drop_last: bool = False,
                 synthetic: Union[bool, str] = "auto", synthetic_size: int = 60000, device_augment: bool = False,
                 hflip: float = 0.0, rand_augment_ops: int = 0, rand_augment_magnitude: int = 9,
                 rand_augment_fill: int = 0):
        self.hparams = dict(channels_last=channels_last, random_crop=random_crop, data_dir=data_dir, val_split=val_split,
                            num_workers=num_workers, normalize=normalize, pin_memory=pin_memory, batch_size=batch_size,
                            seed=seed, synthetic=synthetic)
        self.device_augment = bool(device_augment)
        self.augment = None
        ra = _rand_augment(self.hparams, self.device_augment, (28, 28), rand_augment_ops, rand_augment_magnitude,
                           rand_augment_fill)
        if self.device_augment:
            if not channels_last:
                raise ValueError("device_augment=True needs channels_last=True (ops.batch_augment writes channels-last)")
            self.hparams.update(device_augment=True, hflip=hflip)
            side = random_crop or 28
            self.augment = DeviceAugment((28, 28), (side, side), mode="random_crop", hflip=hflip,
                                         mean=(0.5,) if normalize else (0.0,), std=(0.5,) if normalize else (1.0,),
                                         rand_augment=ra)
        self.channels_last, self.random_crop = channels_last, random_crop
        self.data_dir = data_dir or "."
        self.val_split, self.num_workers, self.normalize = val_split, num_workers, normalize
        self.pin_memory, self.batch_size, self.seed = pin_memory, batch_size, seed
        self.shuffle, self.drop_last = shuffle, drop_last
        self.synthetic, self.synthetic_size = synthetic, synthetic_size
        self.num_classes = 10
        side = random_crop or 28
        self._image_shape = (side, side, 1) if channels_last else (1, side, side)
        self.ds_train = self.ds_val = self.ds_test = None

    @property
    def image_shape(self):
        return self._image_shape

    @property
    def dims(self):
        return (1, self._image_shape[0], self._image_shape[1]) if self.channels_last else self._image_shape

    def _use_synthetic(self) -> bool:
        if self.synthetic == "auto":
            return _find(self.data_dir, "train-images-idx3-ubyte") is None
        return bool(self.synthetic)

    def prepare_data(self):
        if not self._use_synthetic() and _find(self.data_dir, "train-images-idx3-ubyte") is None:
            raise FileNotFoundError(f"MNIST IDX files not found under {self.data_dir} (offline; use --data.synthetic=true)")

    def setup(self, stage: Optional[str] = None):
        if self._use_synthetic():
            n = self.synthetic_size
            full = SyntheticImages(n, (28, 28, 1), 10, seed=self.seed)
            imgs = torch.stack([((full[i][0][..., 0] * 0.5 + 0.5) * 255).round().to(torch.uint8) for i in range(n)])
            labs = torch.tensor([full[i][1] for i in range(n)])
            timgs, tlabs = imgs[: max(1, n // 6)], labs[: max(1, n // 6)]
        else:
            imgs = _read_idx(_find(self.data_dir, "train-images-idx3-ubyte"))
            labs = _read_idx(_find(self.data_dir, "train-labels-idx1-ubyte")).long()
            timgs = _read_idx(_find(self.data_dir, "t10k-images-idx3-ubyte"))
            tlabs = _read_idx(_find(self.data_dir, "t10k-labels-idx1-ubyte")).long()
        n = len(labs)
        nval = int(self.val_split * n) if isinstance(self.val_split, float) else min(int(self.val_split), n // 2)
        g = torch.Generator().manual_seed(self.seed)
        perm = torch.randperm(n, generator=g)
        tr, va = perm[: n - nval], perm[n - nval:]
        if self.device_augment:
            mk = lambda i, l, train: _RawImages(i, l)
        else:
            mk = lambda i, l, train: _Transformed(i, l, self.random_crop, self.normalize, self.channels_last, train)
        self.ds_train = mk(imgs[tr], labs[tr], True)
        self.ds_val = mk(imgs[va], labs[va], False)
        self.ds_test = mk(timgs, tlabs, False)

    def _dl(self, ds, shuffle):
        return torch.utils.data.DataLoader(ds, batch_size=self.batch_size, shuffle=shuffle, num_workers=self.num_workers,
                                           pin_memory=self.pin_memory, drop_last=self.drop_last,
                                           persistent_workers=self.num_workers > 0)

    def train_dataloader(self):
        return self._dl(self.ds_train, self.shuffle)

    def val_dataloader(self):
        return self._dl(self.ds_val, False)

    def test_dataloader(self):
        return self._dl(self.ds_test, False)


class _AsUint8(torch.utils.data.Dataset):
    """Images in [-1, 1] of another dataset as raw uint8 (0..255), the format of a decoded image file."""

    def __init__(self, ds):
        self.ds = ds

    def __len__(self):
        return len(self.ds)

    def __getitem__(self, i):
        x, y = self.ds[i]
        return ((x * 0.5 + 0.5) * 255.0).round().to(torch.uint8), y


@register_datamodule
class SyntheticImageDataModule:
    """ImageNet-shape (224×224×3 by default) synthetic classification data (BASELINE config 4)."""

    def __init__(self, image_shape=(224, 224, 3), num_classes: int = 1000, size: int = 10000, batch_size: int = 32,
                 num_workers: int = 2, pin_memory: bool = False, seed: int = 0, device_augment: bool = False,
                 source_shape=None, scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3), hflip: float = 0.5,
                 rand_augment_ops: int = 0, rand_augment_magnitude: int = 9, rand_augment_fill: int = 0):
        """``device_augment=True``: uint8 sources of ``source_shape`` (default: ``image_shape`` + 32
        rows and columns), random-resized-cropped to ``image_shape``, flipped and normalized on
        the device (``self.augment``); ``rand_augment_ops > 0``: that many RandAugment layers on
        the source first."""
        self.hparams = dict(image_shape=list(image_shape), num_classes=num_classes, size=size, batch_size=batch_size)
        self._image_shape = tuple(image_shape)
        self.num_classes = num_classes
        self.size, self.batch_size, self.num_workers, self.pin_memory, self.seed = size, batch_size, num_workers, pin_memory, seed
        self.device_augment = bool(device_augment)
        self.augment = None
        if not self.device_augment:  # raises when RandAugment is asked for
            _rand_augment(self.hparams, False, None, rand_augment_ops, rand_augment_magnitude, rand_augment_fill)
        if self.device_augment:
            h, w, c = self._image_shape
            self.source_shape = tuple(source_shape) if source_shape is not None else (h + 32, w + 32, c)
            if len(self.source_shape) != 3 or self.source_shape[2] != c:
                raise ValueError(f"source_shape {self.source_shape} must be (Hs, Ws, {c})")
            ra = _rand_augment(self.hparams, True, self.source_shape[:2], rand_augment_ops, rand_augment_magnitude,
                               rand_augment_fill)
            self.hparams.update(device_augment=True, source_shape=list(self.source_shape), scale=list(scale),
                                ratio=list(ratio), hflip=hflip)
            self.augment = DeviceAugment(self.source_shape[:2], (h, w), mode="random_resized_crop", scale=tuple(scale),
                                         ratio=tuple(ratio), hflip=hflip, mean=(0.5,), std=(0.5,), rand_augment=ra)

    @property
    def image_shape(self):
        return self._image_shape

    def prepare_data(self):
        pass

    def setup(self, stage=None):
        shape = self.source_shape if self.device_augment else self._image_shape
        self.ds_train = SyntheticImages(self.size, shape, self.num_classes, seed=self.seed)
        self.ds_val = SyntheticImages(max(64, self.size // 10), shape, self.num_classes, seed=self.seed + 1)
        if self.device_augment:
            self.ds_train, self.ds_val = _AsUint8(self.ds_train), _AsUint8(self.ds_val)

    def _dl(self, ds, shuffle):
        return torch.utils.data.DataLoader(ds, batch_size=self.batch_size, shuffle=shuffle, num_workers=self.num_workers,
                                           pin_memory=self.pin_memory)

    def train_dataloader(self):
        return self._dl(self.ds_train, True)

    def val_dataloader(self):
        return self._dl(self.ds_val, False)

    def test_dataloader(self):
        return self._dl(self.ds_val, False)


@register_datamodule
class NpyImageDataModule:
    """A pre-decoded image dataset in ``data_dir``: ``train_images.npy`` ``(N, Hs, Ws, C)`` (or
    ``(N, Hs, Ws)``) uint8, ``train_labels.npy`` ``(N,)`` integers, and ``val_images.npy`` /
    ``val_labels.npy``, memory-mapped (no image library).  Always the device path: the loaders yield
    raw uint8 batches and ``self.augment`` (``mode``: ``random_resized_crop`` or ``random_crop``)
    crops / resizes to ``image_shape``, flips and normalizes on the device."""

    def __init__(self, data_dir: str, image_shape=(224, 224, 3), num_classes: int = 1000, batch_size: int = 32,
                 num_workers: int = 2, pin_memory: bool = False, shuffle: bool = True, drop_last: bool = False,
                 mode: str = "random_resized_crop", scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3), hflip: float = 0.5,
                 eval_crop_pct: float = 0.875, mean=(0.5,), std=(0.5,), rand_augment_ops: int = 0,
                 rand_augment_magnitude: int = 9, rand_augment_fill: int = 0):
        self.hparams = dict(data_dir=data_dir, image_shape=list(image_shape), num_classes=num_classes,
                            batch_size=batch_size, mode=mode, scale=list(scale), ratio=list(ratio), hflip=hflip,
                            eval_crop_pct=eval_crop_pct, mean=list(mean), std=list(std))
        self.data_dir = data_dir
        self._image_shape = tuple(image_shape)
        self.num_classes = num_classes
        self.batch_size, self.num_workers, self.pin_memory = batch_size, num_workers, pin_memory
        self.shuffle, self.drop_last = shuffle, drop_last
        self.device_augment = True
        self._aug = dict(mode=mode, scale=tuple(scale), ratio=tuple(ratio), hflip=hflip, eval_crop_pct=eval_crop_pct,
                         mean=tuple(mean), std=tuple(std))
        self.augment = None  # built in setup(): the source size comes from the files
        # validated (and recorded in hparams) now; the RandAugment itself needs the source size too
        self._ra = (int(rand_augment_ops), int(rand_augment_magnitude), int(rand_augment_fill))
        if self._ra[0] > 0:
            _rand_augment(self.hparams, True, (1, 1), *self._ra)
        self.ds_train = self.ds_val = None

    @property
    def image_shape(self):
        return self._image_shape

    def _path(self, name: str) -> str:
        return os.path.join(self.data_dir, name)

    def prepare_data(self):
        for name in ("train_images.npy", "train_labels.npy", "val_images.npy", "val_labels.npy"):
            if not os.path.exists(self._path(name)):
                raise FileNotFoundError(f"{name} not found under {self.data_dir}")

    def _load(self, split: str):
        import numpy as np

        imgs = np.load(self._path(f"{split}_images.npy"), mmap_mode="r")
        labs = np.load(self._path(f"{split}_labels.npy")).astype(np.int64)
        c = self._image_shape[2]
        if imgs.dtype != np.uint8 or imgs.ndim not in (3, 4) or (imgs.shape[3] if imgs.ndim == 4 else 1) != c:
            raise ValueError(f"{split}_images.npy must be (N, Hs, Ws{', ' + str(c) if c > 1 else '[, 1]'}) uint8, "
                             f"got {imgs.shape} {imgs.dtype}")
        if labs.shape != (imgs.shape[0],):
            raise ValueError(f"{split}_labels.npy must be ({imgs.shape[0]},), got {labs.shape}")
        return imgs, labs

    def setup(self, stage=None):
        timgs, tlabs = self._load("train")
        vimgs, vlabs = self._load("val")
        if timgs.shape[1:3] != vimgs.shape[1:3]:
            raise ValueError(f"train {timgs.shape[1:3]} and val {vimgs.shape[1:3]} image sizes differ")
        self.augment = DeviceAugment(timgs.shape[1:3], self._image_shape[:2], **self._aug,
                                     rand_augment=_rand_augment({}, True, timgs.shape[1:3], *self._ra))
        self.ds_train, self.ds_val = _RawImages(timgs, tlabs), _RawImages(vimgs, vlabs)

    def _dl(self, ds, shuffle):
        return torch.utils.data.DataLoader(ds, batch_size=self.batch_size, shuffle=shuffle, num_workers=self.num_workers,
                                           pin_memory=self.pin_memory, drop_last=self.drop_last and shuffle,
                                           persistent_workers=self.num_workers > 0)

    def train_dataloader(self):
        return self._dl(self.ds_train, self.shuffle)

    def val_dataloader(self):
        return self._dl(self.ds_val, False)

    def test_dataloader(self):
        return self._dl(self.ds_val, False)
