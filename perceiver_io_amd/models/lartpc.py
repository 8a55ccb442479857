"""LArTPC per-pixel segmentation model (reference ``run.py:72-124``) and its sparse
execution.

The reference runs Perceiver IO densely on a 512×512 wire-plane image: 262,144 keys through the
encoder cross-attention (K/V LayerNorm + projection for every pixel), with the zero pixels
masked as keys (``mask = x == 0``, ``run.py:117``), and 262,144 output queries per sample
through the decoder, followed by a class-weighted cross-entropy whose background weight is 0
(``run.py:238-241``).  About 1–3 % of the pixels are non-zero, so nearly all of that work is
discarded.

``LArPerceiver.sparse_loss`` computes the same loss and gradients from the pixels that matter:

* **encoder**: masked keys get exactly zero attention weight, so the encoder output depends
  only on the non-zero pixels.  Their ``[pixel ‖ Fourier PE]`` rows are gathered (the PE by flat
  pixel index, ``sparse_inputs``) and the encoder runs over those keys alone,
  with the padding of the per-batch capacity masked.
* **decoder**: a pixel whose class weight is 0 contributes nothing to the loss, so its output
  query receives a zero gradient.  Only the queries of weighted pixels are decoded
  (``PerceiverDecoder.hidden_at``), and the cross-entropy is the weighted mean over them.

Parameter gradients (including the zero rows of the 262,144 × C output-query table) equal the
dense computation's.  ``tests/test_lartpc.py`` checks this against the dense eager model.
``forward`` keeps the dense per-pixel logits of the reference.

Inference runs sparse too: ``LArPerceiver.segment`` compacts a dense event to its non-zero pixels
on the device, encodes those, decodes the same pixels and writes their classes into a uint8
class map (``segment_sparse`` takes already sparse operands).  The class of a lit pixel equals the
dense model's ``argmax``; unlit pixels read as background, which is what the reference displays.
"""
from __future__ import annotations

from typing import Dict, NamedTuple, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

from .adapters import ClassificationOutputAdapter, ImageInputAdapter
from .perceiver import PerceiverDecoder, PerceiverEncoder, PerceiverIO
from .uresnet import UResNet

NUM_CLASSES = 3
CLASS_WEIGHTS = (0.0, 1.0, 1.0)  # background, track, shower (reference run.py:238-240)


class SegLoss(NamedTuple):
    """The segmentation loss of :func:`ops.pixel_head.pixel_seg_loss`: ``ce_weight`` · focal
    cross-entropy (``focal_gamma`` = 0: the weighted cross-entropy) + ``dice_weight`` · soft Dice."""

    focal_gamma: float = 0.0
    ce_weight: float = 1.0
    dice_weight: float = 0.0
    dice_eps: float = 1.0


class Segmentation(NamedTuple):
    """Result of :meth:`LArPerceiver.segment` / :meth:`LArPerceiver.segment_sparse`."""

    classes: torch.Tensor              # (B, Q) uint8: class of each query pixel, 0 on padding slots
    confidence: torch.Tensor           # (B, Q) fp32: softmax probability of that class, 0 on padding
    class_map: torch.Tensor            # (B, H·W) uint8: the classes at their pixels, 0 elsewhere
    confusion: Optional[torch.Tensor]  # (3, 3) int64, rows = label, columns = prediction (with labels)
    count: torch.Tensor                # (B,) int32: non-zero pixels per sample (may exceed the capacity)


def sparse_inputs(adapter: ImageInputAdapter, values: torch.Tensor, index: torch.Tensor) -> torch.Tensor:
    """``[pixel channels ‖ Fourier PE]`` rows at flat pixel positions ``index`` (B, K):
    ``values`` (B, K, C_img) → (B, K, Kin), the rows ``adapter(x)`` has at those positions."""
    pe = adapter.position_encoding
    b, k = index.shape
    rows = pe.index_select(0, index.reshape(-1)).view(b, k, pe.shape[1])
    return torch.cat([values.to(pe.dtype).view(b, k, -1), rows], dim=-1)


class LArPerceiver(torch.nn.Module):
    """The reference ``LAr_Perceiver`` (``run.py:72-124``): Fourier-encoded 512×512×1 input,
    32×64 latents, 3 × (1 cross + 3 self-attention) layers with 4 heads, a 1-head decoder with
    one output query per pixel and a 3-way classifier.  The U-ResNet is built alongside, unused in
    ``forward``, as in the reference (its parameters stay in the state dict)."""

    def __init__(self, size: int = 512, latents: Tuple[int, int] = (32, 64), bands: int = 32):
        super().__init__()
        n, c = latents
        enc = PerceiverEncoder(ImageInputAdapter((size, size, 1), bands), (n, c), num_layers=3,
                               num_cross_attention_heads=4, num_self_attention_heads=4,
                               num_self_attention_layers_per_block=3, dropout=0.0)
        dec = PerceiverDecoder(ClassificationOutputAdapter(num_classes=NUM_CLASSES, num_outputs=size * size,
                                                           num_output_channels=c),
                               (n, c), num_cross_attention_heads=1, dropout=0.0)
        self.size = size
        self.perceiver = PerceiverIO(enc, dec)
        self.uresnet = UResNet(num_classes=NUM_CLASSES, input_channels=c, inplanes=16)

    @property
    def encoder(self) -> PerceiverEncoder:
        return self.perceiver.encoder

    @property
    def decoder(self) -> PerceiverDecoder:
        return self.perceiver.decoder

    def trained_parameters(self):
        """The parameters that receive gradients (the unused U-ResNet excluded)."""
        return list(self.perceiver.parameters())

    def forward(self, img):
        """Dense per-pixel logits ``(B, 3, H·W)`` (the reference's output, with the D6 permute fix)."""
        b = img.shape[0]
        x = img.reshape(b, self.size, self.size, 1)
        mask = (x == 0).reshape(b, -1)  # zero pixels are padding keys
        logits = self.perceiver(x, mask)  # (B, H*W, 3)
        return logits.permute(0, 2, 1)

    def sparse_hidden(self, values, index, kmask, qidx):
        """Decoder output ``(B, K', C)`` at output pixels ``qidx``, from the non-zero pixels only."""
        from .. import ops

        enc, dec = self.perceiver.encoder, self.perceiver.decoder
        if ops.use_hip(enc.latent):  # PE rows read at `index` inside the K/V projection kernels
            lat = ops.fused.encode_sparse(enc, values, index, kmask)
        else:
            lat = enc.forward_inputs(sparse_inputs(enc.input_adapter, values, index), kmask)
        return dec.hidden_at(lat, qidx)

    def sparse_logits(self, values, index, kmask, qidx):
        """Logits ``(B, K', 3)`` at output pixels ``qidx`` from the non-zero pixels only."""
        return self.perceiver.decoder.output_adapter.linear(self.sparse_hidden(values, index, kmask, qidx))

    def sparse_loss(self, batch, weights: torch.Tensor,
                    loss: Optional[SegLoss] = None) -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
        """``(loss, {acc, acc1, acc2})`` for a :func:`data.lartpc.sparse_collate` batch: the
        weighted mean cross-entropy of the dense model (ignored slots are -100) and the
        reference's per-class accuracies, as device tensors.  On the GPU the 3-way head, the
        loss and the accuracies are one fused kernel each way (``ops/pixel_head.py``).

        ``loss`` (a :class:`SegLoss`) selects focal cross-entropy + soft Dice instead
        (``pixel_seg_loss``; the metrics gain ``focal``, ``dice``, ``dice1``, ``dice2``).  Only pixels
        with a positive class weight take part in it, so it too equals its dense computation."""
        from ..ops.pixel_head import pixel_ce, pixel_seg_loss

        values, index, kmask, qidx, qlab = batch
        h = self.sparse_hidden(values, index, kmask, qidx)
        if loss is None:
            return pixel_ce(h, self.perceiver.decoder.output_adapter.linear, qlab, weights)
        return pixel_seg_loss(h, self.perceiver.decoder.output_adapter.linear, qlab, weights, *loss)

    def event_loss(self, batch, weights: torch.Tensor, key_capacity: int, query_capacity: int,
                   class_weights: Sequence[float] = CLASS_WEIGHTS, loss: Optional[SegLoss] = None):
        """``(loss, {acc, acc1, acc2}, counts)`` for dense events ``batch = (img (B, H, W) fp32, lab
        (B, H·W) uint8, words (B,) int32)``: ``ops.event_compact`` builds the sparse batch on the
        batch's device, each sample under the dihedral code in ``words``, and :meth:`sparse_loss`
        takes it from there.  ``class_weights`` is the host copy of ``weights`` (which pixels are
        queries is decided without reading the device).  Shapes depend on the capacities alone, so
        one captured graph serves every batch.  Pixels past a capacity are left out of the loss, as
        in ``segment(capacity=)``; ``counts`` (B, 2) int32 holds the true key and query counts, so
        the caller can see that.  ``loss``: as in :meth:`sparse_loss`."""
        from .. import ops

        img, lab, words = batch
        *sparse, counts = ops.event_compact(img, lab, words, int(key_capacity), int(query_capacity), class_weights)
        value, acc = self.sparse_loss(tuple(sparse), weights, loss)
        return value, acc, counts

    def segment_sparse(self, values, index, kmask, qidx=None, qmask=None, labels=None) -> Segmentation:
        """Class map of a sparse batch (``sparse_collate`` layout, or :func:`nonzero_compact`'s).

        With ``qidx=None`` the queries are the keys: every lit pixel is classified (``qidx =
        index``, valid where ``~kmask``).  Otherwise ``qidx`` (B, Q) names the pixels to classify and
        ``qmask`` (B, Q) bool is True on its padding slots (None: all valid).  ``labels`` (B, Q)
        int64 at the query pixels add the confusion matrix.  The valid query pixels of one sample
        must be distinct (see ``ops.pixel_head.pixel_predict``).  Runs under ``no_grad``: the
        sparse encoder and decoder, then one fused head pass; dense logits never exist."""
        from ..ops.pixel_head import pixel_predict

        with torch.no_grad():
            if qidx is None:
                qidx, qvalid = index, ~kmask
            else:
                qvalid = ~qmask if qmask is not None else torch.ones_like(qidx, dtype=torch.bool)
            h = self.sparse_hidden(values, index, kmask, qidx)
            classes, conf, cmap, confusion = pixel_predict(h, self.perceiver.decoder.output_adapter.linear, qidx, qvalid,
                                                           self.size * self.size, labels)
            return Segmentation(classes, conf, cmap, confusion, (~kmask).sum(1).to(torch.int32))

    def segment(self, img, capacity: Optional[int] = None, bucket: int = 2048, labels=None) -> Segmentation:
        """Class map ``(B, H·W)`` uint8 of dense events ``img`` (B, H, W) or (B, H·W): the class of
        every non-zero pixel, 0 elsewhere (what the reference displays, ``argmax · (x != 0)``).

        The image is compacted to its non-zero pixels (on the GPU by ``nonzero_compact``, in flat
        order, exactly the operands ``sparse_collate`` builds) and goes through
        :meth:`segment_sparse`.  ``capacity=None`` sizes the key set from the data: one counting
        pass, then ``count.max()`` is read on the host — the only synchronisation — and rounded up
        to ``bucket`` so that shapes repeat.  With ``capacity`` given nothing waits on the device;
        pixels past the capacity are not classified, and ``Segmentation.count`` (the true number of
        non-zero pixels per sample) lets the caller detect that.  Dense ``labels`` (B, H·W) are
        gathered at the classified pixels for the confusion matrix."""
        from .. import ops
        from ..data.lartpc import _round_up

        b = img.shape[0]
        flat = img.reshape(b, -1).float().contiguous()
        kern = ops.fused.kernels(flat) if ops.use_hip(flat) else ops.emulation
        if capacity is None:
            count = kern.nonzero_compact(flat, 0)[3]
            capacity = _round_up(int(count.max()), bucket)
        values, index, kmask, count = kern.nonzero_compact(flat, int(capacity))
        qlab = labels.reshape(b, -1).long().gather(1, index) if labels is not None else None
        seg = self.segment_sparse(values, index, kmask, labels=qlab)
        return seg._replace(count=count)

    @torch.no_grad()
    def attention_map(self, img, capacity: Optional[int] = None, bucket: int = 2048, layer: int = 0) -> torch.Tensor:
        """``(B, H·W)`` fp32: the attention mass each pixel receives in the encoder's cross-attention
        application ``layer`` (0 = ``layer_1``, then ``layer_n``'s applications), 0 at unlit pixels.

        The event is compacted as in :meth:`segment` (same ``capacity`` rules, the same single host
        read when ``capacity=None``), only the lit pixels are encoded under
        ``ops.record_attention``, and the mass of the chosen application is scattered to the pixel
        positions.  A sample's map sums to the latent count (0 for an event without lit pixels);
        pixels past the capacity stay 0.  The decoder does not run.

        Eager backends only: the encoder runs through its layer modules in fp32, where the weights
        come from the materialised per-head softmax of the lit keys (``B × H × latents × capacity``
        floats), not from the ``attn_weights`` kernel.  The fused encoder executor is not recorded
        (``ops.record_attention``); with it selected this method raises before doing any work."""
        from .. import ops
        from ..data.lartpc import _round_up

        enc = self.perceiver.encoder
        if ops.use_hip(enc.latent):  # before any work: the refusal costs nothing
            raise RuntimeError("attention_map: the fused encoder is not recorded; run under ops.backend('torch')")
        b = img.shape[0]
        flat = img.reshape(b, -1).float().contiguous()
        kern = ops.emulation  # the eager backend's compaction (use_hip is false here)
        if capacity is None:
            count = kern.nonzero_compact(flat, 0)[3]
            capacity = _round_up(int(count.max()), bucket)
        values, index, kmask, _ = kern.nonzero_compact(flat, int(capacity))
        with ops.record_attention(enc, "mass") as rec:
            enc.forward_inputs(sparse_inputs(enc.input_adapter, values, index), kmask)
        if not 0 <= layer < len(rec.entries):
            raise ValueError(f"attention_map: layer must be in [0, {len(rec.entries)}), got {layer}")
        mass = rec.entries[layer]["tensor"]  # (B, capacity), exactly 0 on the padding slots
        return torch.zeros_like(flat).scatter_add_(1, index, mass.to(flat.dtype))


def iou(confusion: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(per-class IoU (K,), mean IoU)`` of a confusion matrix (rows = label, columns =
    prediction): ``TP / (label + predicted − TP)``; NaN for a class that occurs in neither, and
    the mean runs over the classes present."""
    c = confusion.double()
    tp = c.diagonal()
    union = c.sum(0) + c.sum(1) - tp
    per = torch.where(union > 0, tp / union.clamp(min=1), torch.full_like(tp, float("nan")))
    return per, per[union > 0].mean() if bool((union > 0).any()) else per.new_tensor(float("nan"))


def accuracies(pred: torch.Tensor, lab: torch.Tensor) -> Dict[str, torch.Tensor]:
    """Per-class accuracies of the reference (``run.py:190-206``) as device tensors: over labelled
    pixels (label > 0), tracks (1) and showers (2); 0 where a class is absent."""
    out = {}
    for name, sel in (("acc", lab > 0), ("acc1", lab == 1), ("acc2", lab == 2)):
        n = sel.sum()
        hit = ((pred == lab) & sel).sum()
        out[name] = torch.where(n > 0, hit.float() / n.clamp(min=1).float(), torch.zeros((), device=lab.device))
    return out


def class_weights(device, weights: Sequence[float] = CLASS_WEIGHTS) -> torch.Tensor:
    return torch.tensor(list(weights), dtype=torch.float32, device=device)
