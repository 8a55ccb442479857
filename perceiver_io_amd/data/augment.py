"""Host-side parameter draws for the device-side image augmentation (``ops.batch_augment``).

The data loader delivers raw ``uint8`` batches; per training step the task module draws one
``(B, 8)`` float32 block ``{y0, x0, h, w, flip, 0, 0, 0}`` per sample here (numpy, vectorised over
the batch — no per-sample Python) and the kernel crops, resizes, flips and normalizes on the
device.  On the captured-graph path the block travels inside the batch and is staged into the
graph's static inputs, like the MixUp / CutMix words.

Modes:
  * ``random_crop`` — a box of exactly ``out_hw`` at uniform integer offsets (training) or centred
    (evaluation): the MNIST ``RandomCrop`` transform of ``data/mnist.py``.  The kernel takes its
    copy path, bit for bit the host transform.
  * ``random_resized_crop`` — torchvision ``RandomResizedCrop.get_params``: up to 10 attempts per
    sample (all drawn at once, the first valid taken), area fraction uniform in ``scale``, aspect
    ratio log-uniform in ``ratio``, ``w = round(√(A·r))``, ``h = round(√(A/r))``, valid when the box
    fits; otherwise the centred whole-image crop with its ratio clamped into ``ratio``.
    Evaluation: the centred box spanning ``eval_crop_pct`` of the shorter side with the aspect
    ratio of ``out_hw`` (resize-then-centre-crop).
``flip ~ Bernoulli(hflip)`` per sample in training, never in evaluation.
"""
from __future__ import annotations

import math
from typing import Sequence, Tuple

import numpy as np
import torch

MODES = ("random_crop", "random_resized_crop")
ATTEMPTS = 10


class DeviceAugment:
    def __init__(self, source_hw: Tuple[int, int], out_hw: Tuple[int, int], mode: str = "random_crop",
                 scale: Tuple[float, float] = (0.08, 1.0), ratio: Tuple[float, float] = (3 / 4, 4 / 3),
                 hflip: float = 0.0, eval_crop_pct: float = 0.875, mean: Sequence[float] = (0.5,),
                 std: Sequence[float] = (0.5,)):
        if mode not in MODES:
            raise ValueError(f"mode must be one of {MODES}, got {mode!r}")
        self.source_hw = (int(source_hw[0]), int(source_hw[1]))
        self.out_hw = (int(out_hw[0]), int(out_hw[1]))
        if min(self.source_hw + self.out_hw) < 1:
            raise ValueError(f"source_hw {source_hw} and out_hw {out_hw} must be positive")
        if mode == "random_crop" and (self.out_hw[0] > self.source_hw[0] or self.out_hw[1] > self.source_hw[1]):
            raise ValueError(f"random_crop: out_hw {self.out_hw} must fit into source_hw {self.source_hw}")
        self.mode = mode
        self.scale = (float(scale[0]), float(scale[1]))
        self.ratio = (float(ratio[0]), float(ratio[1]))
        if not (0.0 < self.scale[0] <= self.scale[1]) or not (0.0 < self.ratio[0] <= self.ratio[1]):
            raise ValueError(f"scale {scale} and ratio {ratio} must be positive (min, max) pairs")
        self.hflip = float(hflip)
        self.eval_crop_pct = float(eval_crop_pct)
        self.mean = [float(m) for m in (mean if isinstance(mean, (list, tuple)) else [mean])]
        self.std = [float(s) for s in (std if isinstance(std, (list, tuple)) else [std])]

    # -- boxes -----------------------------------------------------------------------------------
    def fallback_box(self) -> Tuple[int, int, int, int]:
        """The centred whole-image crop with its aspect ratio clamped into ``ratio`` → (y0, x0, h, w)."""
        H, W = self.source_hw
        in_ratio = W / H
        if in_ratio < self.ratio[0]:
            w, h = W, int(round(W / self.ratio[0]))
        elif in_ratio > self.ratio[1]:
            h, w = H, int(round(H * self.ratio[1]))
        else:
            h, w = H, W
        h, w = min(max(h, 1), H), min(max(w, 1), W)
        return (H - h) // 2, (W - w) // 2, h, w

    def eval_box(self) -> Tuple[int, int, int, int]:
        H, W = self.source_hw
        oh, ow = self.out_hw
        if self.mode == "random_crop":
            h, w = oh, ow
        else:
            side = self.eval_crop_pct * min(H, W)
            h, w = (side * oh / ow, side) if ow >= oh else (side, side * ow / oh)
            h, w = min(max(int(round(h)), 1), H), min(max(int(round(w)), 1), W)
        return (H - h) // 2, (W - w) // 2, h, w

    def draw(self, rng: np.random.Generator, B: int, train: bool = True) -> np.ndarray:
        """One block of per-sample words ``(B, 8)`` float32 from the ``numpy.random.Generator``."""
        out = np.zeros((B, 8), dtype=np.float32)
        if not train:
            out[:, :4] = self.eval_box()
            return out
        H, W = self.source_hw
        if self.mode == "random_crop":
            oh, ow = self.out_hw
            out[:, 0] = rng.integers(0, H - oh + 1, size=B)
            out[:, 1] = rng.integers(0, W - ow + 1, size=B)
            out[:, 2], out[:, 3] = oh, ow
        else:
            area = H * W * rng.uniform(self.scale[0], self.scale[1], size=(B, ATTEMPTS))
            r = np.exp(rng.uniform(math.log(self.ratio[0]), math.log(self.ratio[1]), size=(B, ATTEMPTS)))
            w = np.rint(np.sqrt(area * r)).astype(np.int64)
            h = np.rint(np.sqrt(area / r)).astype(np.int64)
            ok = (w > 0) & (w <= W) & (h > 0) & (h <= H)
            first = ok.argmax(axis=1)
            rows = np.arange(B)
            fy, fx, fh, fw = self.fallback_box()
            any_ok = ok.any(axis=1)
            h = np.where(any_ok, h[rows, first], fh)
            w = np.where(any_ok, w[rows, first], fw)
            u = rng.random(size=(B, 2))  # uniform integer offsets in [0, H − h] × [0, W − w]
            y0 = np.minimum((u[:, 0] * (H - h + 1)).astype(np.int64), H - h)
            x0 = np.minimum((u[:, 1] * (W - w + 1)).astype(np.int64), W - w)
            out[:, 0] = np.where(any_ok, y0, fy)
            out[:, 1] = np.where(any_ok, x0, fx)
            out[:, 2], out[:, 3] = h, w
        if self.hflip > 0.0:
            out[:, 4] = rng.random(size=B) < self.hflip
        return out

    # -- device ----------------------------------------------------------------------------------
    def apply(self, x_u8: torch.Tensor, params) -> torch.Tensor:
        """``ops.batch_augment`` of a raw ``(B, Hs, Ws, C)`` uint8 batch with drawn ``params``."""
        from .. import ops

        if not torch.is_tensor(params):
            params = torch.from_numpy(np.ascontiguousarray(params, dtype=np.float32))
        return ops.batch_augment(x_u8, params.to(x_u8.device), self.mean, self.std, self.out_hw)
