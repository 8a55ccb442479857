"""Op layer: hand-written HIP/CDNA4 kernels (``perceiver_io_amd/csrc``) behind
autograd Functions, plus the eager PyTorch oracle used on CPU and in tests.

Backend selection (``PERCEIVER_BACKEND`` env or :func:`set_backend`):
  * ``auto``  — HIP kernels for CUDA(HIP) tensors, eager PyTorch on CPU.  On a GPU
    box a missing/broken extension raises instead of silently falling back.
  * ``hip``   — force the kernels (error if unavailable).
  * ``torch`` — eager PyTorch everywhere (this framework's own eager oracle).
  * ``reference`` — eager PyTorch with the reference's exact compute: ``nn.MultiheadAttention``
    math (``F.multi_head_attention_forward``, need_weights=True), full ``(B, V, L)`` logits
    cross-entropy and sync-ing boolean-index masking.  Used to measure the baseline.
"""
from __future__ import annotations

import os
from contextlib import contextmanager

import torch

from . import ext  # noqa: F401  (extension loader)

_BACKEND = os.environ.get("PERCEIVER_BACKEND", "auto")
_VALID = ("auto", "hip", "torch", "reference")


def set_backend(name: str) -> None:
    global _BACKEND
    if name not in _VALID:
        raise ValueError(f"backend must be one of {_VALID}, got {name!r}")
    _BACKEND = name


def get_backend() -> str:
    return _BACKEND


@contextmanager
def backend(name: str):
    prev = get_backend()
    set_backend(name)
    try:
        yield
    finally:
        set_backend(prev)


_DETERMINISTIC = [False]


def set_deterministic(flag: bool) -> None:
    """Deterministic mode (trainer ``deterministic=True``): every kernel reduction
    that would use fp32 atomics with several writers per address runs as a fixed-order split
    reduction, so identical runs give bitwise-identical parameters."""
    _DETERMINISTIC[0] = bool(flag)
    if ext.available():
        ext.require().set_deterministic(bool(flag))


def deterministic() -> bool:
    return _DETERMINISTIC[0]


def check_device_errors(reset: bool = True) -> None:
    """Read the kernels' sticky device error words (one host sync) and raise on any.

    * ``csrc/persist.hip`` ``sa_block_fwd``: a bounded spin that timed out (bit 0: a tile gave up
      waiting for its sample's next-layer Q/K/V rows and computed on whatever was there) or an
      invalid tile ticket (bit 1).  The launch finishes either way (no GPU hang); this turns the
      corrupted forward into an error instead of silent training on garbage.
    * checked builds (``PERCEIVER_CHECKED=1``): the index-validation words — token ids, gather
      rows and class labels outside their tables (the kernels clamped / skipped the access), and
      bit 16: a ``batch_augment`` crop box that reached outside its source image (clamped; the
      call itself never raises for it), bit 32: a ``rand_augment`` op word outside its table
      (applied as identity), and bit 64: a chunk of ``adamw_grouped`` outside the flat buffers, or
      a group id of ``adamw_grouped`` / ``lamb(tensor_group=)`` outside the optimizer's groups (the
      chunk is skipped; ``lamb`` skips a chunk outside the buffers without flagging it), and bit
      128: an ``event_compact`` dihedral code outside 0–7 (applied as identity; a label at or past
      the class count raises bit 4 and is not selected).
      Outside a graph capture every checked launch raises at once (``checked_sync``); inside a
      replayed hipGraph nothing can.

    Called by the Trainer at every logging step and at the end of ``fit`` and by ``bench.py``
    after its timed loop (SURVEY §5.3 failure detection)."""
    if not ext.available() or not torch.cuda.is_available() or not torch.cuda.is_initialized():
        return
    K = ext.require()
    e = int(K.persist_errors(reset))
    if e:
        what = []
        if e & 1:
            what.append("a bounded spin timed out: a tile computed on rows its sample had not published")
        if e & 2:
            what.append("a workgroup drew a tile ticket outside the grid")
        raise RuntimeError(f"sa_block_fwd_kernel (csrc/persist.hip) device error word {e:#x}: " + "; ".join(what)
                           + ".  The persistent self-attention block forward's results of that step are invalid")
    if K.checked_build():
        c = int(K.check_errors(reset))
        if c:
            raise RuntimeError(f"checked build: out-of-range indices seen on the device (error bits {c:#x}: "
                               "1 token id >= vocab, 2 gather row out of range, 4 label outside [0, V) and != -100, "
                               "8 PE row index outside the position-encoding table, "
                               "16 batch_augment crop box outside its source image, "
                               "32 rand_augment op word outside its table, "
                               "64 adamw_grouped chunk outside the flat buffers, or an optimizer group id outside its groups, "
                               "128 event_compact dihedral code outside 0-7)")


def use_hip(t: torch.Tensor) -> bool:
    """True when ``t`` should be processed by the HIP kernels."""
    if _BACKEND in ("torch", "reference") or not t.is_cuda:
        return False
    ext.require()  # raises loudly if the extension is missing on a GPU
    return True


MIX_OFF, MIX_MIXUP, MIX_CUTMIX = 0, 1, 2


def batch_mix(x: torch.Tensor, y: torch.Tensor, mix: torch.Tensor):
    """MixUp / CutMix of a channels-last image batch ``x`` (B, H, W, Ch) with its flipped self
    (sample i pairs with sample B − 1 − i) → ``(mixed, label_b, lam)``; ``x`` is not modified.
    ``mix`` holds the fp32 words ``{mode, λ, y0, y1, x0, x1}`` (mode 0 off, 1 MixUp, 2 CutMix with
    the partner's pixels inside rows [y0, y1) × columns [x0, x1)) on ``x``'s device.  HIP path:
    one kernel that reads ``mix`` from device memory (``csrc/soft_ce_head.hip``) — no host sync,
    and a replayed hipGraph mixes with whatever words were staged for that step."""
    y = y if y.dtype == torch.int64 and y.is_contiguous() else y.to(torch.int64).contiguous()
    if use_hip(x):
        xc = x if x.dtype == torch.float32 and x.is_contiguous() else x.float().contiguous()
        m = mix.to(device=x.device, dtype=torch.float32).contiguous()
        out, yb, lam = ext.require().batch_mix(xc, y, m)
        return out, yb, lam
    from . import emulation

    return emulation.batch_mix(x, y, mix)


def _per_channel(v, C: int):
    vals = [float(a) for a in (v if isinstance(v, (list, tuple)) else torch.as_tensor(v).reshape(-1).tolist())]
    if len(vals) == 1:
        vals = vals * C
    if len(vals) != C:
        raise ValueError(f"batch_augment: mean / std need 1 or {C} values, got {len(vals)}")
    return vals


def batch_augment(src: torch.Tensor, params: torch.Tensor, mean, std, out_hw) -> torch.Tensor:
    """Crop → bilinear resize → horizontal flip → normalize of a raw ``uint8`` channels-last batch
    ``src`` (B, Hs, Ws, C ≤ 4) → fp32 (B, out_h, out_w, C).  ``params`` (B, 8) fp32 holds per sample
    ``{y0, x0, h, w, flip, 0, 0, 0}``: the crop box in source pixels (integers stored as floats)
    and the flip flag (≥ 0.5: mirrored columns); ``mean`` / ``std``: one value per channel (or one
    for all).  Same values as ``F.interpolate(box, out_hw, mode="bilinear", align_corners=False)``
    → flip → ``(v / 255 − mean) / std``; a box of the output size is copied without any
    interpolation arithmetic, bit for bit the host pipeline's result.  The box is clamped into
    the source in every build.  HIP path: one kernel that reads ``params`` from device memory
    (``csrc/augment.hip``) — no host sync, and a replayed hipGraph augments with whatever words
    were staged for that step."""
    if src.dtype != torch.uint8 or src.dim() != 4:
        raise ValueError(f"batch_augment: src must be a (B, Hs, Ws, C) uint8 batch, got {tuple(src.shape)} {src.dtype}")
    C = src.shape[3]
    mean, std = _per_channel(mean, C), _per_channel(std, C)
    if use_hip(src):
        p = params.to(device=src.device, dtype=torch.float32).contiguous()
        return ext.require().batch_augment(src.contiguous(), p, mean, std, int(out_hw[0]), int(out_hw[1]))
    from . import emulation

    return emulation.batch_augment(src, params, mean, std, out_hw)


def rand_augment(src: torch.Tensor, words: torch.Tensor, fill: int = 0) -> torch.Tensor:
    """RandAugment of a raw ``uint8`` channels-last batch ``src`` (B, H, W, C ∈ {1, 3}) → uint8 of the
    same shape.  ``words`` (B, N, 8) fp32 holds per sample and layer ``{op, v, m00, m01, m02, m10,
    m11, m12}`` (``data.augment.RandAugment.draw``): op 0 identity, 1 nearest-neighbour affine with
    the inverse matrix ``m`` in the pixel-centre convention (outside → ``fill``), 2 brightness,
    3 color, 4 contrast, 5 sharpness (factor ``v``), 6 posterize (``v`` bits), 7 solarize (threshold
    ``v``), 8 autocontrast, 9 equalize; the layers run in order on uint8 intermediates.  An op word
    outside the table is identity.  HIP path: two kernels per layer that read ``words`` from device
    memory (``csrc/randaugment.hip``) — no host sync, and a replayed hipGraph augments with
    whatever words were staged for that step; bit for bit ``emulation.rand_augment``."""
    if src.dtype != torch.uint8 or src.dim() != 4 or src.shape[3] not in (1, 3) or not src.is_contiguous():
        raise ValueError("rand_augment: src must be a contiguous (B, H, W, C) uint8 batch with 1 or 3 channels, got "
                         f"{tuple(src.shape)} {src.dtype}")
    if words.dim() != 3 or words.shape[0] != src.shape[0] or words.shape[1] < 1 or words.shape[2] != 8:
        raise ValueError(f"rand_augment: words must be (B, N >= 1, 8), got {tuple(words.shape)}")
    if not 0 <= int(fill) <= 255:
        raise ValueError(f"rand_augment: fill must be a uint8 value, got {fill}")
    if use_hip(src):
        w = words.to(device=src.device, dtype=torch.float32).contiguous()
        return ext.require().rand_augment(src, w, int(fill))
    from . import emulation

    return emulation.rand_augment(src, words, int(fill))


def event_compact(img: torch.Tensor, lab: torch.Tensor, words: torch.Tensor, key_cap: int, query_cap: int, weights):
    """Dense LArTPC events → the sparse training batch of ``data.lartpc.sparse_collate`` at fixed
    capacities, read through one dihedral symmetry per sample.

    ``img`` (B, H, W) fp32, ``lab`` (B, H·W) uint8 and ``words`` (B,) int32 live on one device.  Code
    bits: 4 transposes first ((i', j') = (j, i)), 1 mirrors the columns (j' = W − 1 − j'), 2 the rows
    (i' = H − 1 − i'), where output pixel (i, j) takes source pixel (i', j'); a code outside 0–7 is
    the identity (the checked build flags it).  ``weights``: the class weights as a Python sequence
    of at most 8 floats; a pixel is a query when its label's weight is non-zero.  Returns ``(values
    (B, key_cap, 1), index (B, key_cap) int64, kmask (B, key_cap) bool, qidx (B, query_cap) int64,
    qlab (B, query_cap) int64, counts (B, 2) int32)`` in the flat order of the transformed event,
    padded exactly like ``sparse_collate``; ``counts`` holds the true key and query counts, also
    beyond the capacities (capacities 0 only count).

    HIP path: ``csrc/lartpc_prep.hip`` reads ``words`` from device memory — no host sync, and a
    replayed hipGraph transforms with whatever words were staged for that step.  Because the host
    never sees the words, it refuses non-square planes outright: a transposing code needs H == W.
    The emulation (CPU) takes non-square planes and raises only when a word transposes."""
    weights = tuple(float(w) for w in weights)
    if not 1 <= len(weights) <= 8:
        raise ValueError(f"event_compact: 1 to 8 class weights, got {len(weights)}")
    if img.dim() != 3 or lab.shape != (img.shape[0], img.shape[1] * img.shape[2]) or lab.dtype != torch.uint8:
        raise ValueError(f"event_compact: img (B, H, W) and lab (B, H*W) uint8, got {tuple(img.shape)} and "
                         f"{tuple(lab.shape)} {lab.dtype}")
    if words.shape != (img.shape[0],):
        raise ValueError(f"event_compact: words must be (B,), got {tuple(words.shape)}")
    wmask = sum(1 << c for c, w in enumerate(weights) if w != 0)
    if use_hip(img):
        if img.shape[1] != img.shape[2]:
            raise ValueError(f"event_compact: the device path needs square planes, got {tuple(img.shape[1:])}")
        x = img if img.dtype == torch.float32 and img.is_contiguous() else img.float().contiguous()
        w = words.to(device=img.device, dtype=torch.int32).contiguous()
        return tuple(ext.require().event_compact(x, lab.contiguous(), w, int(key_cap), int(query_cap), wmask, len(weights)))
    from . import emulation

    return tuple(emulation.event_compact(img.float(), lab, words, int(key_cap), int(query_cap), wmask, len(weights)))


from . import attention, fused, masking, mlm_head, optim  # noqa: E402,F401
from .attention import attention_mass, attention_weights, record_attention  # noqa: E402,F401
