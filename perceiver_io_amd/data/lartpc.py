"""Sparse batches for the LArTPC experiment (``models/lartpc.py``).

A LArTPC wire-plane image is ~1–3 % non-zero.  ``sparse_collate`` turns dense events
``(image (H, W), labels (H·W,))`` into fixed-capacity sparse tensors, on the CPU inside the
DataLoader workers:

* ``values`` (B, K, 1) float32 — the non-zero pixel values, ``index`` (B, K) int64 — their flat
  positions, ``kmask`` (B, K) bool — True on capacity padding (masked keys);
* ``qidx`` (B, Q) int64 — the pixels with a non-zero class weight (the only ones the weighted
  loss sees), ``qlab`` (B, Q) int64 — their labels, -100 on padding.

K and Q are the batch maxima rounded up to a multiple of ``bucket``.  That gives a handful of
distinct shapes, so the step engine keeps one captured hipGraph per shape.

For inference the key tensors are built on the device instead: the ``nonzero_compact`` kernel
(``LArPerceiver.segment``) returns, at the same capacity, bitwise the ``values / index / kmask``
of ``sparse_collate`` from a dense image batch that is already on the GPU.

Training can build the whole batch there (``run.py --device-collate``): ``DenseCollator`` only
stacks the events (fp32 image, uint8 labels), ``DihedralAugment.draw`` adds one int32 code per
sample, and ``ops.event_compact`` (``LArPerceiver.event_loss``) produces all five tensors at fixed
capacities inside the step, read through the flip / 90° turn the code names.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np
import torch

from ..models.lartpc import CLASS_WEIGHTS


def _round_up(n: int, m: int) -> int:
    return max(m, -(-n // m) * m)


def sparse_collate(events: List[Tuple[torch.Tensor, torch.Tensor]], bucket: int = 2048,
                   weights: Sequence[float] = CLASS_WEIGHTS):
    w = torch.tensor(list(weights))
    keys, queries = [], []
    for img, lab in events:
        flat = img.reshape(-1)
        nz = torch.nonzero(flat != 0).squeeze(1)
        keys.append((flat[nz], nz))
        q = torch.nonzero(w[lab.reshape(-1)] > 0).squeeze(1)
        queries.append((q, lab.reshape(-1)[q]))
    b = len(events)
    K = _round_up(max(len(k[1]) for k in keys), bucket)
    Q = _round_up(max(len(q[0]) for q in queries), bucket)
    values = torch.zeros(b, K, 1)
    index = torch.zeros(b, K, dtype=torch.long)
    kmask = torch.ones(b, K, dtype=torch.bool)
    # unused query slots point at distinct pixels (their zero gradients then never pile onto one
    # row of the output-query table in the gather's backward)
    npix = events[0][1].numel()
    qidx = (torch.arange(Q) % npix).repeat(b, 1)
    qlab = torch.full((b, Q), -100, dtype=torch.long)
    for i, ((v, nz), (q, ql)) in enumerate(zip(keys, queries)):
        n, m = len(nz), len(q)
        values[i, :n, 0] = v
        index[i, :n] = nz
        kmask[i, :n] = False
        qidx[i, :m] = q
        qlab[i, :m] = ql
    return values, index, kmask, qidx, qlab


class SparseCollator:
    """Picklable ``collate_fn`` for DataLoader workers."""

    def __init__(self, bucket: int = 2048, weights: Sequence[float] = CLASS_WEIGHTS):
        self.bucket, self.weights = bucket, tuple(weights)

    def __call__(self, events):
        return sparse_collate(events, self.bucket, self.weights)


class DenseCollator:
    """Picklable ``collate_fn`` of the device path: ``(img (B, H, W) fp32, lab (B, H·W) uint8)``.
    Nothing is searched or compacted on the host; labels travel as bytes."""

    def __call__(self, events):
        img = torch.stack([e[0] for e in events]).float()
        lab = torch.stack([e[1].reshape(-1) for e in events]).to(torch.uint8)
        return img, lab


DIHEDRAL_MODES = ("dihedral", "flip", "none")


class DihedralAugment:
    """Flips and 90° turns of a wire-plane event, as one code per sample for
    ``ops.event_compact``: bit 2 transposes (applied first), bit 0 mirrors the columns, bit 1 the
    rows.  ``dihedral`` draws all eight symmetries of the square, ``flip`` bits 0–1 only (the four
    that exist for a non-square plane), ``none`` always 0."""

    def __init__(self, mode: str = "dihedral"):
        if mode not in DIHEDRAL_MODES:
            raise ValueError(f"mode must be one of {DIHEDRAL_MODES}, got {mode!r}")
        self.mode = mode

    @staticmethod
    def rng(seed: int = 0, rank: int = 0) -> np.random.Generator:
        return np.random.default_rng([int(seed), int(rank)])

    def draw(self, rng: np.random.Generator, B: int, train: bool = True) -> np.ndarray:
        """One int32 code per sample; ``train=False`` (evaluation): all zeros."""
        if not train or self.mode == "none":
            return np.zeros(B, dtype=np.int32)
        return rng.integers(0, 8 if self.mode == "dihedral" else 4, size=B).astype(np.int32)

    @staticmethod
    def apply_host(img: torch.Tensor, lab: torch.Tensor, code: int):
        """The transform on the host: ``(img (H, W), lab (H·W,))`` → the same pair under ``code``."""
        from ..ops.emulation import dihedral

        h, w = img.shape
        return dihedral(img, code).contiguous(), dihedral(lab.reshape(h, w), code).reshape(-1).contiguous()
