"""Per-pixel classification head + class-weighted cross-entropy (SURVEY K-17) over the HIP
kernels of ``csrc/pixel_head.hip``.

``pixel_ce(h, linear, labels, weights)`` returns the loss of
``F.cross_entropy(linear(h), labels, weight=weights, ignore_index=-100)`` together with the
per-class accuracies of the LArTPC experiment (reference ``run.py:190-206``).  Logits never
reach memory: the forward pass reads each row of ``h`` once and writes per-block partial sums.
The backward pass reads it again and writes ``dH`` plus per-block ``dW | db`` partials, which are
summed in a fixed order (deterministic).

``pixel_seg_loss`` adds the two losses of unbalanced segmentation on the same row pass: focal
cross-entropy and soft Dice (``pixel_seg_fwd`` / ``pixel_seg_bwd``; the definition is in
``csrc/pixel_head.hip``).  Its parameters are constants of a run, so a captured graph bakes them in.

``pixel_predict`` is the inference counterpart: class, confidence, the per-sample class map and
an optional confusion matrix from the same single pass over ``h``.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch
import torch.nn.functional as F

from . import ext


def _supported(h, w) -> bool:
    from . import use_hip

    return use_hip(h) and h.shape[-1] in (32, 64, 128) and 2 <= w.shape[0] <= 4


class _PixelCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, w, b, labels, wts):
        from .fused import kernels

        K = kernels(h)
        h2 = h.reshape(-1, h.shape[-1]).float().contiguous()
        lab = labels.reshape(-1).contiguous()
        stats, loss = K.pixel_ce_fwd(h2, w.contiguous(), b.contiguous(), lab, wts.float().contiguous())
        ctx.save_for_backward(h2, lab, wts, stats)
        ctx.w, ctx.b, ctx.hshape = w, b, h.shape
        ctx.mark_non_differentiable(stats)
        ctx.set_materialize_grads(False)  # no zero-filled gradient for the statistics output
        return loss, stats

    @staticmethod
    def backward(ctx, g, _gstats):
        from .fused import kernels

        if g is None:
            return None, None, None, None, None
        K = kernels(g)
        h2, lab, wts, stats = ctx.saved_tensors
        w, b = ctx.w, ctx.b
        grads = []
        for p in (w, b):  # accumulated in place: flat-buffer gradient views stay bound
            if p.grad is None:
                p.grad = torch.zeros_like(p)
            grads.append(p.grad if p.requires_grad else torch.zeros_like(p))
        dh = torch.empty_like(h2)
        K.pixel_ce_bwd(h2, w.contiguous(), b.contiguous(), lab, wts.float().contiguous(), g.float().reshape(1).contiguous(),
                       stats, dh, grads[0], grads[1])
        return dh.view(ctx.hshape), None, None, None, None


def _metrics(stats: torch.Tensor, K: int) -> Dict[str, torch.Tensor]:
    ns = 4 + 2 * K
    out = {"acc": stats[ns]}
    for k in range(1, K):
        out[f"acc{k}"] = stats[ns + k]
    return out


def pixel_ce(h: torch.Tensor, linear: torch.nn.Linear, labels: torch.Tensor,
             weights: torch.Tensor) -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
    """(weighted mean CE, {acc, acc1, …}) of ``linear(h)`` against ``labels`` (-100 ignored);
    ``acc`` over labels > 0, ``acc<k>`` over label k (device tensors, no host sync)."""
    K = linear.weight.shape[0]
    if _supported(h, linear.weight):
        loss, stats = _PixelCE.apply(h, linear.weight, linear.bias, labels, weights)
        return loss, _metrics(stats, K)
    logits = linear(h).reshape(-1, K).float()
    lab = labels.reshape(-1)
    loss = F.cross_entropy(logits, lab, weight=weights, ignore_index=-100)
    return loss, _accuracies(logits.argmax(-1), lab, K)


def _accuracies(pred: torch.Tensor, lab: torch.Tensor, K: int) -> Dict[str, torch.Tensor]:
    out = {}
    for name, sel in [("acc", lab > 0)] + [(f"acc{k}", lab == k) for k in range(1, K)]:
        n = sel.sum()
        hit = ((pred == lab) & sel).sum()
        out[name] = torch.where(n > 0, hit.float() / n.clamp(min=1).float(), torch.zeros((), device=lab.device))
    return out


class _PixelSeg(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, w, b, labels, wts, params):
        from .fused import kernels

        K = kernels(h)
        h2 = h.reshape(-1, h.shape[-1]).float().contiguous()
        lab = labels.reshape(-1).contiguous()
        stats, loss = K.pixel_seg_fwd(h2, w.contiguous(), b.contiguous(), lab, wts.float().contiguous(), *params)
        ctx.save_for_backward(h2, lab, wts, stats)
        ctx.w, ctx.b, ctx.hshape, ctx.params = w, b, h.shape, params
        ctx.mark_non_differentiable(stats)
        ctx.set_materialize_grads(False)  # no zero-filled gradient for the statistics output
        return loss, stats

    @staticmethod
    def backward(ctx, g, _gstats):
        from .fused import kernels

        if g is None:
            return None, None, None, None, None, None
        K = kernels(g)
        h2, lab, wts, stats = ctx.saved_tensors
        w, b = ctx.w, ctx.b
        grads = []
        for p in (w, b):  # accumulated in place: flat-buffer gradient views stay bound
            if p.grad is None:
                p.grad = torch.zeros_like(p)
            grads.append(p.grad if p.requires_grad else torch.zeros_like(p))
        dh = torch.empty_like(h2)
        K.pixel_seg_bwd(h2, w.contiguous(), b.contiguous(), lab, wts.float().contiguous(), *ctx.params,
                        g.float().reshape(1).contiguous(), stats, dh, grads[0], grads[1])
        return dh.view(ctx.hshape), None, None, None, None, None


def seg_loss_logits(logits: torch.Tensor, labels: torch.Tensor, weights: torch.Tensor, focal_gamma: float = 0.0,
                    ce_weight: float = 1.0, dice_weight: float = 0.0,
                    dice_eps: float = 1.0) -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
    """:func:`pixel_seg_loss` of logits (R, K) that already exist: the definition as a plain autograd
    composition in fp32 (the dense path, the CPU, and head shapes without a kernel)."""
    from .emulation import check_seg_params

    check_seg_params(focal_gamma, ce_weight, dice_weight, dice_eps)
    K = logits.shape[-1]
    z = logits.reshape(-1, K).float()
    lab = labels.reshape(-1)
    valid = (lab >= 0) & (lab < K)
    labc = lab.clamp(0, K - 1)
    oh = F.one_hot(labc, K).to(z.dtype)
    logp = F.log_softmax(z, -1)
    p = logp.exp()
    wl = torch.where(valid, weights.to(z.dtype)[labc], torch.zeros((), dtype=z.dtype, device=z.device))
    take = valid & (wl > 0)
    zero = torch.zeros((), dtype=z.dtype, device=z.device)
    focal, dice, per = zero, zero, torch.zeros(K, dtype=z.dtype, device=z.device)
    if ce_weight > 0:
        ce = -(logp * oh).sum(-1)
        if focal_gamma > 0:  # q^γ with q clamped off 0: a saturated row has a zero, not an infinite, slope
            q = (p * (1 - oh)).sum(-1).clamp(min=torch.finfo(z.dtype).tiny)
            ce = ce * (q * q if focal_gamma == 2 else q.pow(focal_gamma))
        focal = torch.where(take, wl * ce, zero).sum() / wl.sum()
    if dice_weight > 0:
        pm, om = p * take[:, None], oh * take[:, None]
        per = (2 * (pm * om).sum(0) + dice_eps) / (pm.sum(0) + om.sum(0) + dice_eps)
        S = (weights > 0).to(z.dtype)
        dice = 1 - (per * S).sum() / S.sum()
    loss = (ce_weight * focal if ce_weight > 0 else 0) + (dice_weight * dice if dice_weight > 0 else 0)
    out = _accuracies(z.argmax(-1), lab, K)
    out.update(focal=focal.detach(), dice=dice.detach())
    out.update({f"dice{k}": per[k].detach() for k in range(1, K)})
    return loss, out


def pixel_seg_loss(h: torch.Tensor, linear: torch.nn.Linear, labels: torch.Tensor, weights: torch.Tensor,
                   focal_gamma: float = 0.0, ce_weight: float = 1.0, dice_weight: float = 0.0,
                   dice_eps: float = 1.0) -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
    """``(loss, metrics)`` of ``linear(h)`` against ``labels`` (-100 ignored) with

        loss = ce_weight · focal + dice_weight · dice

    ``focal`` is the class-weighted focal cross-entropy ``Σ w·(1 − pt)^γ·(−log pt) / Σ w`` (γ = 0: the
    loss of :func:`pixel_ce`); ``dice`` is 1 minus the mean soft Dice coefficient
    ``(2·Σ p_c·[y = c] + ε) / (Σ p_c + Σ [y = c] + ε)`` of the classes with a positive weight.  Only
    rows whose label has a positive weight take part, so a sparse batch and the dense one agree.
    ``metrics`` holds the ``acc…`` keys of :func:`pixel_ce` plus ``focal``, ``dice`` and the per-class
    coefficients ``dice1 … dice<K-1>`` (device tensors, no host sync).  A term whose weight is 0 is not
    evaluated and reads 0, its coefficients too.  γ >= 0, both weights >= 0 and not both 0, ε > 0."""
    from .emulation import check_seg_params

    check_seg_params(focal_gamma, ce_weight, dice_weight, dice_eps)
    K = linear.weight.shape[0]
    if not _supported(h, linear.weight):
        return seg_loss_logits(linear(h), labels, weights, focal_gamma, ce_weight, dice_weight, dice_eps)
    params = (float(focal_gamma), float(ce_weight), float(dice_weight), float(dice_eps))
    loss, stats = _PixelSeg.apply(h, linear.weight, linear.bias, labels, weights, params)
    ns = 4 + 5 * K
    out = {"acc": stats[ns]}
    for k in range(1, K):
        out[f"acc{k}"] = stats[ns + k]
    out.update(focal=stats[ns + K], dice=stats[ns + K + 1])
    out.update({f"dice{k}": stats[ns + K + 2 + k] for k in range(1, K)})
    return loss, out


def pixel_predict(h: torch.Tensor, linear: torch.nn.Linear, qidx: torch.Tensor, qvalid: torch.Tensor, npix: int,
                  labels: Optional[torch.Tensor] = None):
    """Per-pixel prediction of ``linear(h)`` without logits in memory (``pixel_predict_kernel``).

    ``h`` (B, Q, C): decoder output at the query pixels ``qidx`` (B, Q) int64 (flat pixel index);
    ``qvalid`` (B, Q) bool marks the real queries.  Returns

    * ``classes`` (B, Q) uint8 — argmax class, the lowest class on an exact tie; 0 on invalid rows;
    * ``conf`` (B, Q) fp32 — the softmax probability of that class; 0 on invalid rows;
    * ``class_map`` (B, npix) uint8 — zero (background) except ``class_map[b, qidx[b, q]] =
      classes[b, q]`` for the valid rows.  An index outside [0, npix) is skipped (the row keeps its
      ``classes`` / ``conf`` entry; the checked build raises).  The valid indices of one sample must
      be distinct, as ``sparse_collate`` and ``nonzero_compact`` build them: with duplicates, which
      row's class lands in the map is unspecified;
    * ``confusion`` (K, K) int64, rows = label, columns = prediction, over the valid rows with
      ``0 <= label < K`` — ``None`` without ``labels`` (B, Q) int64.

    No gradient flows through any output."""
    K = linear.weight.shape[0]
    B, Q, C = h.shape
    with torch.no_grad():
        h2 = h.reshape(B * Q, C).float().contiguous()
        idx = qidx.reshape(-1).long().contiguous()
        val = qvalid.reshape(-1).bool().contiguous()
        lab = labels.reshape(-1).long().contiguous() if labels is not None else None
        if _supported(h, linear.weight):
            from .fused import kernels

            kern = kernels(h)
        else:
            from . import emulation as kern
        out = kern.pixel_predict(h2, linear.weight.detach().float().contiguous(), linear.bias.detach().float().contiguous(),
                                 idx, val, Q, int(npix), lab)
        conf = out[3].sum(0, dtype=torch.int64).view(K, K) if lab is not None else None
        return out[0].view(B, Q), out[1].view(B, Q), out[2], conf
