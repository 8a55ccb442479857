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

``RandAugment`` draws the ``(B, num_ops, 8)`` word block of ``ops.rand_augment`` the same way; a
``DeviceAugment`` that carries one (``rand_augment=``) applies it to the raw source batch before
the crop box is taken.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

MODES = ("random_crop", "random_resized_crop")
ATTEMPTS = 10


class DeviceAugment:
    def __init__(self, source_hw: Tuple[int, int], out_hw: Tuple[int, int], mode: str = "random_crop",
                 scale: Tuple[float, float] = (0.08, 1.0), ratio: Tuple[float, float] = (3 / 4, 4 / 3),
                 hflip: float = 0.0, eval_crop_pct: float = 0.875, mean: Sequence[float] = (0.5,),
                 std: Sequence[float] = (0.5,), rand_augment: Optional["RandAugment"] = None):
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
        if rand_augment is not None and rand_augment.source_hw != self.source_hw:
            raise ValueError(f"rand_augment is for {rand_augment.source_hw} sources, this augmenter for {self.source_hw}")
        self.rand_augment = rand_augment

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
    def apply(self, x_u8: torch.Tensor, params, ra_words=None) -> torch.Tensor:
        """``ops.batch_augment`` of a raw ``(B, Hs, Ws, C)`` uint8 batch with drawn ``params``; with
        ``ra_words`` (``self.rand_augment.draw``) ``ops.rand_augment`` runs on the source batch first."""
        from .. import ops

        if not torch.is_tensor(params):
            params = torch.from_numpy(np.ascontiguousarray(params, dtype=np.float32))
        if ra_words is not None:
            if self.rand_augment is None:
                raise ValueError("ra_words given, but this augmenter has no rand_augment")
            if not torch.is_tensor(ra_words):
                ra_words = torch.from_numpy(np.ascontiguousarray(ra_words, dtype=np.float32))
            x_u8 = ops.rand_augment(x_u8.contiguous(), ra_words.to(x_u8.device), self.rand_augment.fill)
        return ops.batch_augment(x_u8, params.to(x_u8.device), self.mean, self.std, self.out_hw)


# the 14 operations of torchvision's RandAugment table in its order → the op code of ops.rand_augment
RA_NAMES = ("Identity", "ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate", "Brightness", "Color", "Contrast",
            "Sharpness", "Posterize", "Solarize", "AutoContrast", "Equalize")
RA_CODES = np.array([0, 1, 1, 1, 1, 1, 2, 3, 4, 5, 6, 7, 8, 9], dtype=np.int64)
_RA_SIGNED = np.array([0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0], dtype=bool)


class RandAugment:
    """Host draws of ``ops.rand_augment``'s words after torchvision's ``RandAugment``: each of
    ``num_ops`` layers picks one of the 14 operations of ``RA_NAMES`` uniformly, at the strength
    the table gives bin ``magnitude`` of ``num_magnitude_bins``: ShearX / ShearY up to 0.3,
    TranslateX / TranslateY up to 150/331 of the width / height (truncated to whole pixels), Rotate
    up to 30° (counter-clockwise for a positive draw), Brightness / Color / Contrast / Sharpness at
    factor 1 ± up to 0.9, Posterize at ``8 − round(m / ((bins − 1) / 4))`` bits, Solarize with the
    threshold falling from 255 to 0, AutoContrast, Equalize.  The signed ones are negated with
    probability ½.  The five geometric operations leave as op 1 with the inverse matrix (output →
    source) composed about the image centre ``(W/2, H/2)`` in the pixel-centre convention (pixel j
    spans [j, j + 1), centre j + 0.5), computed in float64 and stored as fp32."""

    def __init__(self, source_hw: Tuple[int, int], num_ops: int = 2, magnitude: int = 9, num_magnitude_bins: int = 31,
                 fill: int = 0):
        self.source_hw = (int(source_hw[0]), int(source_hw[1]))
        self.num_ops, self.magnitude, self.bins, self.fill = int(num_ops), int(magnitude), int(num_magnitude_bins), int(fill)
        if min(self.source_hw) < 1:
            raise ValueError(f"source_hw {source_hw} must be positive")
        if not 1 <= self.num_ops <= 8:
            raise ValueError(f"num_ops must be in 1..8, got {num_ops}")
        if self.bins < 2 or not 0 <= self.magnitude < self.bins:
            raise ValueError(f"magnitude {magnitude} must be a bin index of num_magnitude_bins {num_magnitude_bins} >= 2")
        if not 0 <= self.fill <= 255:
            raise ValueError(f"fill must be a uint8 value, got {fill}")

    def strengths(self) -> dict:
        """The unsigned table value of every operation at this magnitude (torchvision's
        ``_augmentation_space``)."""
        H, W = self.source_hw
        frac = self.magnitude / (self.bins - 1)
        return {"Identity": 0.0, "ShearX": 0.3 * frac, "ShearY": 0.3 * frac, "TranslateX": 150.0 / 331.0 * W * frac,
                "TranslateY": 150.0 / 331.0 * H * frac, "Rotate": 30.0 * frac, "Brightness": 0.9 * frac,
                "Color": 0.9 * frac, "Contrast": 0.9 * frac, "Sharpness": 0.9 * frac,
                "Posterize": float(8 - int(round(self.magnitude / ((self.bins - 1) / 4)))),
                "Solarize": 255.0 - 255.0 * frac, "AutoContrast": 0.0, "Equalize": 0.0}

    def draw(self, rng: np.random.Generator, B: int, train: bool = True) -> np.ndarray:
        """One block of per-sample words ``(B, num_ops, 8)`` float32: ``{op, v, m00, m01, m02, m10,
        m11, m12}`` per layer; ``train=False``: all identity."""
        N = self.num_ops
        out = np.zeros((B, N, 8), dtype=np.float64)
        out[..., 2] = out[..., 6] = 1.0  # the identity matrix
        if not train:
            return out.astype(np.float32)
        k = rng.integers(0, len(RA_NAMES), size=(B, N))
        neg = rng.integers(0, 2, size=(B, N)).astype(bool) & _RA_SIGNED[k]
        mag = np.array([self.strengths()[n] for n in RA_NAMES], dtype=np.float64)[k]
        mag = np.where(neg, -mag, mag)
        out[..., 0] = RA_CODES[k]
        # v: the blend factor of the four enhancements, the bits / threshold of posterize / solarize
        out[..., 1] = np.where((k >= 6) & (k <= 9), 1.0 + mag, np.where((k == 10) | (k == 11), mag, 0.0))
        # inverse matrix A and translation t about the centre c: source = A·(p − c) + c + t
        H, W = self.source_hw
        cx, cy = W / 2.0, H / 2.0
        th = np.where(k == 5, np.deg2rad(mag), 0.0)
        a00, a11 = np.cos(th), np.cos(th)
        a01 = np.where(k == 1, mag, 0.0 - np.sin(th))
        a10 = np.where(k == 2, mag, np.sin(th))
        tx = np.where(k == 3, -np.trunc(mag), 0.0)
        ty = np.where(k == 4, -np.trunc(mag), 0.0)
        out[..., 2], out[..., 3], out[..., 4] = a00, a01, cx - a00 * cx - a01 * cy + tx
        out[..., 5], out[..., 6], out[..., 7] = a10, a11, cy - a10 * cx - a11 * cy + ty
        return out.astype(np.float32)
