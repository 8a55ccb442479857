"""Task modules: masked language model, text classifier, image classifier.

Reference parity (``perceiver/lightning.py``):
  * ``LitModel``               — ``:29-55``: shared architecture hparams + defaults,
    ``save_hyperparameters``, optimizer / per-step scheduler from ``{class_path, init_args}``.
  * ``LitClassifier``          — ``:58-85``: CE loss + argmax accuracy; logs ``train_loss``,
    ``train_acc``, ``val_loss``, ``val_acc``, ``test_loss``, ``test_acc``.
  * ``LitImageClassifier``     — ``:88-126``.
  * ``LitTextClassifier``      — ``:129-171``: encoder shared with the MLM, transfer from
    ``mlm_ckpt`` (encoder) or ``clf_ckpt`` (whole model), ``freeze_encoder``.  Defect D3
    fixed (``PerceiverIO.encoder`` exists); D8: a stale nested ``mlm_ckpt`` path inside a
    ``clf_ckpt``'s hparams is skipped with a warning instead of crashing.
  * ``LitMaskedLanguageModel`` — ``:174-256``: defect D1 fixed (``TextMasking`` built from
    the tokenizer constants), sample predictions after each validation epoch.

Training loss of the MLM uses ``PerceiverMLM.loss`` (identical value, vocab head only on
selected positions); ``step`` on the ``reference`` backend reproduces the full-logits path.
"""
from __future__ import annotations

import inspect
import os
import warnings
from typing import Any, List, Optional, Tuple

import torch
import torch.nn as nn

from .models import (ClassificationOutputAdapter, ImageInputAdapter, PerceiverDecoder, PerceiverEncoder, PerceiverIO,
                     PerceiverMLM, TextInputAdapter, TextMasking, TextOutputAdapter)
from .train.module import LitModuleBase, import_class, instantiate_class
from .utils.misc import freeze, predict_masked_samples
from .utils.tokenizer import MASK_TOKEN_ID, PAD_TOKEN_ID, SPECIAL_TOKENS, UNK_TOKEN_ID

# text batches are padded to a multiple of this many tokens before a graph-captured step
LENGTH_BUCKET = 64


def bucket_text_batch(batch, max_seq_len: int, multiple: int = LENGTH_BUCKET):
    """``(labels, ids, pad_mask)`` padded along the sequence to ``round_up(L, multiple)``
    (capped at ``max_seq_len``) with PAD ids and ``True`` (= padding) mask entries.

    The reference collator pads each batch to its longest sequence (``data/imdb.py:52-63``), so
    an epoch sees hundreds of lengths; captured step graphs are cached per shape, and this
    bounds the distinct shapes to ``max_seq_len / multiple``.  Semantics are unchanged: padded
    keys are masked out of every cross-attention (K-08), masking never selects PAD positions,
    and the MLM loss / classifier read no padded position."""
    y, x, m = batch
    L = x.shape[1]
    Lp = min(-(-L // multiple) * multiple, max(L, int(max_seq_len)))
    if Lp == L:
        return batch
    if m is None:
        m = torch.zeros(x.shape, dtype=torch.bool, device=x.device)
    x = torch.nn.functional.pad(x, (0, Lp - L), value=PAD_TOKEN_ID)
    m = torch.nn.functional.pad(m, (0, Lp - L), value=True)
    return y, x, m


class LitModel(LitModuleBase):
    def __init__(self,
                 optimizer_init: dict,
                 scheduler_init: Optional[dict] = None,
                 num_latents: int = 64,
                 num_latent_channels: int = 64,
                 num_encoder_layers: int = 3,
                 num_encoder_cross_attention_heads: int = 4,
                 num_encoder_self_attention_heads: int = 4,
                 num_encoder_self_attention_layers_per_block: int = 6,
                 num_decoder_cross_attention_heads: int = 4,
                 dropout: float = 0.0,
                 no_decay_1d: bool = False,
                 encoder_lr_scale: float = 1.0):
        super().__init__()
        self.save_hyperparameters()

    @property
    def latent_shape(self) -> Tuple[int, int]:
        return self.hparams.num_latents, self.hparams.num_latent_channels

    def optimizer_groups(self):
        """The parameter groups of ``no_decay_1d`` / ``encoder_lr_scale`` (``ops.optim.param_groups``
        over ``self.model``, ``lr = optimizer lr · lr_scale`` per group), or None with the defaults
        (checkpoints from before the two options lack them: the defaults)."""
        no_decay = bool(self.hparams.get("no_decay_1d", False))
        scale = self.hparams.get("encoder_lr_scale", 1.0)
        scale = 1.0 if scale is None else float(scale)  # 0 is a value: the encoder stands still
        if not no_decay and scale == 1.0:
            return None
        from .ops.optim import param_groups, scale_group_lrs

        init = self.hparams.optimizer_init
        cls_defaults = inspect.signature(import_class(init["class_path"]).__init__).parameters
        args = dict(init.get("init_args", {}) or {})
        lr = args.get("lr", cls_defaults["lr"].default)
        wd = args.get("weight_decay", cls_defaults["weight_decay"].default)
        enc = getattr(self.model, "encoder", None)
        prefix = next((n + "." for n, m in self.model.named_children() if m is enc), None)
        scales = {prefix: scale} if prefix is not None and scale != 1.0 else None
        groups = param_groups(self.model, wd, no_decay_1d=no_decay, lr_scales=scales)
        seen = {id(p) for g in groups for p in g["params"]}
        rest = [p for p in self.parameters() if p.requires_grad and id(p) not in seen]
        if rest:  # parameters outside self.model: plain options
            groups.append({"params": rest, "weight_decay": float(wd), "lr_scale": 1.0})
        return scale_group_lrs(groups, lr)

    def configure_optimizers(self):
        groups = self.optimizer_groups()
        if groups is not None:
            from .ops.optim import scale_scheduler_init

            optimizer = instantiate_class(groups, self.hparams.optimizer_init)
            if self.hparams.get("scheduler_init") is None:
                return optimizer
            scheduler = instantiate_class(optimizer, scale_scheduler_init(self.hparams.scheduler_init, groups))
            return {"optimizer": optimizer,
                    "lr_scheduler": {"scheduler": scheduler, "interval": "step", "frequency": 1}}
        optimizer = instantiate_class(self.parameters(), self.hparams.optimizer_init)
        if self.hparams.get("scheduler_init") is None:
            return optimizer
        scheduler = instantiate_class(optimizer, self.hparams.scheduler_init)
        return {"optimizer": optimizer,
                "lr_scheduler": {"scheduler": scheduler, "interval": "step", "frequency": 1}}


class Accuracy:
    """argmax accuracy (torchmetrics ``Accuracy`` as used at ``lightning.py:62,68``)."""

    def __call__(self, y_pred: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        return (y_pred == y).float().mean()


class LitClassifier(LitModel):
    def __init__(self, *args: Any, label_smoothing: float = 0.0, **kwargs: Any):
        super().__init__(*args, **kwargs)
        self.loss = nn.CrossEntropyLoss()
        self.acc = Accuracy()

    @property
    def soft_targets(self) -> bool:
        """True when the step runs through the soft-target head (label smoothing; subclasses add
        their mixing options).  False: ``step`` is the plain hard-label step."""
        return float(self.hparams.get("label_smoothing", 0.0) or 0.0) != 0.0

    def step(self, batch):
        if self.soft_targets:
            return self.soft_step(batch)
        logits, y = self(batch)
        loss = self.loss(logits.float(), y)
        acc = self.acc(logits.argmax(dim=-1), y)
        return loss, acc

    def soft_inputs(self, batch):
        """→ (x, pad_mask, label_a, label_b, lam) of a batch for the soft-target step;
        ``label_b`` / ``lam`` None: hard labels."""
        raise NotImplementedError

    def soft_step(self, batch):
        """Loss and accuracy through ``PerceiverIO.soft_loss`` (fused soft-target head on the GPU,
        no logits tensor): ``nn.CrossEntropyLoss(label_smoothing)`` semantics on hard labels, the
        label pair's mixture when a subclass mixed the batch.  Accuracy compares the head's
        argmax with the dominant label (``a`` if λ ≥ 0.5, else ``b``)."""
        x, pad_mask, a, b, lam = self.soft_inputs(batch)
        loss, pred = self.model.soft_loss(x, a, b, lam, label_smoothing=float(self.hparams.get("label_smoothing", 0.0)),
                                          pad_mask=pad_mask)
        y = a if b is None else torch.where(lam >= 0.5, a, b)
        return loss, self.acc(pred, y)

    def training_step(self, batch, batch_idx):
        loss, acc = self.step(batch)
        self.log("train_loss", loss)
        self.log("train_acc", acc, prog_bar=True)
        return loss

    def validation_step(self, batch, batch_idx):
        loss, acc = self.step(batch)
        self.log("val_loss", loss, prog_bar=True)
        self.log("val_acc", acc, prog_bar=True)

    def test_step(self, batch, batch_idx):
        loss, acc = self.step(batch)
        self.log("test_loss", loss)
        self.log("test_acc", acc)


def draw_mix(rng, image_hw: Tuple[int, int], mixup_alpha: float = 0.0, cutmix_alpha: float = 0.0,
             mix_prob: float = 1.0, mix_switch_prob: float = 0.5):
    """One batch-mode MixUp / CutMix draw (timm ``Mixup`` semantics, ``mode="batch"``) from the
    ``numpy.random.Generator`` ``rng`` → the six words ``[mode, λ, y0, y1, x0, x1]`` of
    ``ops.batch_mix``.  With probability ``mix_prob`` the batch is mixed; CutMix is chosen with
    probability ``mix_switch_prob`` when both alphas are > 0; λ ~ Beta(α, α); the CutMix box has
    side ratio √(1 − λ) around a uniform centre, is clipped to the image, and λ is reset to
    ``1 − box_area / (H·W)``."""
    off = [0.0, 1.0, 0.0, 0.0, 0.0, 0.0]
    if (mixup_alpha <= 0.0 and cutmix_alpha <= 0.0) or rng.random() >= mix_prob:
        return off
    if mixup_alpha > 0.0 and cutmix_alpha > 0.0:
        cut = bool(rng.random() < mix_switch_prob)
    else:
        cut = cutmix_alpha > 0.0
    alpha = cutmix_alpha if cut else mixup_alpha
    lam = float(rng.beta(alpha, alpha))
    if not cut:
        return [1.0, lam, 0.0, 0.0, 0.0, 0.0]
    H, W = int(image_hw[0]), int(image_hw[1])
    ratio = (1.0 - lam) ** 0.5
    ch, cw = int(H * ratio), int(W * ratio)
    cy, cx = int(rng.integers(0, H)), int(rng.integers(0, W))
    y0, y1 = min(max(cy - ch // 2, 0), H), min(max(cy + ch // 2, 0), H)
    x0, x1 = min(max(cx - cw // 2, 0), W), min(max(cx + cw // 2, 0), W)
    lam = 1.0 - ((y1 - y0) * (x1 - x0)) / float(H * W)
    return [2.0, lam, float(y0), float(y1), float(x0), float(x1)]


class LitImageClassifier(LitClassifier):
    def __init__(self, image_shape: Tuple[int, int, int], num_classes: int, *args: Any, num_frequency_bands: int = 32,
                 mixup_alpha: float = 0.0, cutmix_alpha: float = 0.0, mix_prob: float = 1.0,
                 mix_switch_prob: float = 0.5, **kwargs: Any):
        super().__init__(*args, **kwargs)
        self.model = self.create_model()
        self._mix_rng = None
        self._aug_rng = None
        self._ra_rng = None
        self.augment = None  # a DeviceAugment set directly (tests); else the data module's

    def create_model(self):
        hp = self.hparams
        input_adapter = ImageInputAdapter(image_shape=tuple(hp.image_shape), num_frequency_bands=hp.num_frequency_bands)
        output_adapter = ClassificationOutputAdapter(num_classes=hp.num_classes, num_output_channels=hp.num_latent_channels)
        encoder = PerceiverEncoder(
            input_adapter=input_adapter, latent_shape=self.latent_shape, num_layers=hp.num_encoder_layers,
            num_cross_attention_heads=hp.num_encoder_cross_attention_heads,
            num_self_attention_heads=hp.num_encoder_self_attention_heads,
            num_self_attention_layers_per_block=hp.num_encoder_self_attention_layers_per_block, dropout=hp.dropout)
        decoder = PerceiverDecoder(output_adapter=output_adapter, latent_shape=self.latent_shape,
                                   num_cross_attention_heads=hp.num_decoder_cross_attention_heads, dropout=hp.dropout)
        return PerceiverIO(encoder, decoder)

    def forward(self, batch):
        x, y, _ = self.inputs(batch)
        return self.model(x), y

    # -- device-side augmentation ---------------------------------------------------------------
    # batch layouts: (x, y), (x, y, mix), (x, y, mix | None, aug) and (x, y, mix | None, aug, ra);
    # ``aug`` is the (B, 8) block of DeviceAugment.draw for a raw uint8 ``x``, ``ra`` the
    # (B, num_ops, 8) block of its RandAugment's draw
    def _host_rng(self, tag: int):
        import numpy as np

        tr = self._trainer
        seed = getattr(tr, "seed", None) if tr is not None else None
        rank = getattr(getattr(tr, "dist", None), "rank", 0) if tr is not None else 0
        base = int(seed) if seed is not None else int(torch.initial_seed() % (1 << 31))
        return np.random.default_rng([base, int(rank), tag])

    @property
    def augmenter(self):
        """The ``DeviceAugment`` of this module: its own ``augment`` attribute, else the trainer's
        data module's."""
        if self.augment is not None:
            return self.augment
        tr = self._trainer
        return getattr(getattr(tr, "datamodule", None), "augment", None) if tr is not None else None

    def draw_augment(self, B: int, train: bool) -> torch.Tensor:
        """This micro-batch's augmentation words as a host tensor, drawn from the module's own
        ``numpy.random.Generator`` (seeded from the trainer seed and rank on first use); the data
        loader's workers draw nothing on this path."""
        if self._aug_rng is None:
            self._aug_rng = self._host_rng(0x415547)
        return torch.from_numpy(self._require_augmenter().draw(self._aug_rng, int(B), train))

    def draw_rand_augment(self, B: int, train: bool = True) -> torch.Tensor:
        """This micro-batch's RandAugment words as a host tensor, from a generator of their own
        (same seeding scheme as ``draw_augment``)."""
        if self._ra_rng is None:
            self._ra_rng = self._host_rng(0x52414E44)
        return torch.from_numpy(self._require_augmenter().rand_augment.draw(self._ra_rng, int(B), train))

    def _require_augmenter(self):
        aug = self.augmenter
        if aug is None:
            raise RuntimeError("the batch holds raw uint8 images but there is no augmenter: use a data module with "
                               "device_augment=true (its `augment`), or set the module's `augment` attribute")
        return aug

    def inputs(self, batch):
        """→ (x fp32, y, mix words or None) of a batch: a raw uint8 ``x`` goes through
        ``ops.batch_augment`` first, with the words the batch carries (graph path) or a draw made
        here (eager path; the evaluation draw outside training)."""
        x, y = batch[0], batch[1]
        mix = batch[2] if len(batch) > 2 else None
        if x.dtype == torch.uint8:
            augmenter = self._require_augmenter()
            aug = batch[3] if len(batch) > 3 else None
            if aug is None:
                aug = self.draw_augment(x.shape[0], self.training)
            if getattr(augmenter, "rand_augment", None) is None:
                x = augmenter.apply(x, aug)
            else:  # eager evaluation: no RandAugment call at all
                ra = batch[4] if len(batch) > 4 else None
                if ra is None and self.training:
                    ra = self.draw_rand_augment(x.shape[0])
                x = augmenter.apply(x, aug, ra)
        return x, y, mix

    # -- MixUp / CutMix ------------------------------------------------------------------------
    @property
    def mixing(self) -> bool:
        hp = self.hparams
        return float(hp.get("mixup_alpha", 0.0) or 0.0) > 0.0 or float(hp.get("cutmix_alpha", 0.0) or 0.0) > 0.0

    @property
    def soft_targets(self) -> bool:
        return super().soft_targets or self.mixing

    def draw_mix(self) -> torch.Tensor:
        """This micro-batch's mix words as a host tensor: one draw from the module's own
        ``numpy.random.Generator``, seeded from the trainer seed (rank-shifted) on first use."""
        if self._mix_rng is None:
            self._mix_rng = self._host_rng(0x4D4958)
        hp = self.hparams
        return torch.tensor(draw_mix(self._mix_rng, tuple(hp.image_shape)[:2], float(hp.get("mixup_alpha", 0.0)),
                                     float(hp.get("cutmix_alpha", 0.0)), float(hp.get("mix_prob", 1.0)),
                                     float(hp.get("mix_switch_prob", 0.5))), dtype=torch.float32)

    def graph_batch(self, batch):
        """Graph path: the host draws travel inside the batch — ``(x, y, mix)`` when mixing,
        ``(x, y, mix | None, aug)`` for a raw uint8 ``x``, ``(x, y, mix | None, aug, ra)`` when the
        augmenter has a RandAugment — so the step engine stages them into the captured graph's
        static inputs and every replay mixes / augments with fresh values."""
        if len(batch) != 2:
            return batch
        x, y = batch
        mix = self.draw_mix().to(x.device, non_blocking=True) if self.mixing else None
        if x.dtype == torch.uint8:
            aug = self.draw_augment(x.shape[0], True).to(x.device, non_blocking=True)
            if getattr(self._require_augmenter(), "rand_augment", None) is None:
                return x, y, mix, aug
            return x, y, mix, aug, self.draw_rand_augment(x.shape[0]).to(x.device, non_blocking=True)
        return batch if mix is None else (x, y, mix)

    def soft_inputs(self, batch):
        x, y, mix = self.inputs(batch)
        if not (self.training and self.mixing):  # validation / test: hard labels, never mixed
            return x, None, y, None, None
        if mix is None:
            mix = self.draw_mix().to(x.device)  # eager path: drawn here
        from . import ops

        xm, yb, lam = ops.batch_mix(x, y, mix)
        return xm, None, y, yb, lam


class LitTextClassifier(LitClassifier):
    def __init__(self, num_classes: int, vocab_size: int, max_seq_len: int, *args: Any, freeze_encoder: bool = False,
                 mlm_ckpt: Optional[str] = None, clf_ckpt: Optional[str] = None, **kwargs: Any):
        super().__init__(*args, **kwargs)
        encoder = LitMaskedLanguageModel.create_encoder(self.hparams, self.latent_shape)
        self.model = self.create_model(encoder)
        if mlm_ckpt is not None:
            lit = LitMaskedLanguageModel.load_from_checkpoint(mlm_ckpt)
            self.model.encoder.load_state_dict(lit.model.encoder.state_dict())
        elif clf_ckpt is not None:
            lit = LitTextClassifier.load_from_checkpoint(clf_ckpt, **_stale_ckpt_overrides(clf_ckpt))
            self.model.load_state_dict(lit.model.state_dict())
        if freeze_encoder:
            freeze(self.model.encoder)

    def create_model(self, encoder):
        hp = self.hparams
        output_adapter = ClassificationOutputAdapter(num_classes=hp.num_classes, num_output_channels=hp.num_latent_channels)
        decoder = PerceiverDecoder(output_adapter=output_adapter, latent_shape=self.latent_shape,
                                   num_cross_attention_heads=hp.num_decoder_cross_attention_heads, dropout=hp.dropout)
        return PerceiverIO(encoder, decoder)

    def forward(self, batch):
        y, x, x_mask = batch
        return self.model(x, x_mask), y

    def soft_inputs(self, batch):
        y, x, x_mask = batch
        return x, x_mask, y, None, None

    def graph_batch(self, batch):
        return bucket_text_batch(batch, self.hparams.max_seq_len)


def _stale_ckpt_overrides(clf_ckpt: str) -> dict:
    """D8: the clf checkpoint's hparams may carry an mlm_ckpt path that no longer exists."""
    from .train.checkpoint import load_checkpoint

    hp = load_checkpoint(clf_ckpt, map_location="cpu").get("hyper_parameters", {})
    nested = hp.get("mlm_ckpt")
    if nested and not os.path.exists(nested):
        warnings.warn(f"clf_ckpt refers to missing mlm_ckpt {nested!r}; skipping the nested encoder load")
        return {"mlm_ckpt": None}
    return {}


class LitMaskedLanguageModel(LitModel):
    def __init__(self, vocab_size: int, max_seq_len: int, *args: Any, masked_samples: Optional[List[str]] = None,
                 num_predictions: int = 3, whole_word_masking: bool = False, mask_p: float = 0.15,
                 word_clump: float = 2.0, tokenizer_path: Optional[str] = None, **kwargs: Any):
        """``whole_word_masking``: select whole words (``TextMasking(whole_word=True)``) with the
        continuation table of the WordPiece tokenizer at ``tokenizer_path`` (default: the packaged
        tokenizer of ``vocab_size``); ``word_clump`` then sizes the loss's selection capacity (Σ len² /
        Σ len over the words of the corpus, ``utils.tokenizer.word_clump``; unused otherwise).
        ``mask_p``: the masking rate.  Checkpoints from before these options load with the defaults."""
        super().__init__(*args, **kwargs)
        self.model = self.create_model()
        self.loss = nn.CrossEntropyLoss()

    @staticmethod
    def create_encoder(hparams, latent_shape):
        input_adapter = TextInputAdapter(vocab_size=hparams.vocab_size, max_seq_len=hparams.max_seq_len,
                                         num_input_channels=hparams.num_latent_channels)
        return PerceiverEncoder(
            input_adapter=input_adapter, latent_shape=latent_shape, num_layers=hparams.num_encoder_layers,
            num_cross_attention_heads=hparams.num_encoder_cross_attention_heads,
            num_self_attention_heads=hparams.num_encoder_self_attention_heads,
            num_self_attention_layers_per_block=hparams.num_encoder_self_attention_layers_per_block,
            dropout=hparams.dropout)

    def create_model(self):
        hp = self.hparams
        encoder = self.create_encoder(hp, self.latent_shape)
        output_adapter = TextOutputAdapter(vocab_size=hp.vocab_size, max_seq_len=hp.max_seq_len,
                                           num_output_channels=hp.num_latent_channels)
        decoder = PerceiverDecoder(output_adapter=output_adapter, latent_shape=self.latent_shape,
                                   num_cross_attention_heads=hp.num_decoder_cross_attention_heads, dropout=hp.dropout)
        whole_word = bool(hp.get("whole_word_masking", False))
        masking = TextMasking(hp.vocab_size, unk_token_id=UNK_TOKEN_ID, mask_token_id=MASK_TOKEN_ID,
                              num_special_tokens=len(SPECIAL_TOKENS), mask_p=hp.get("mask_p", 0.15),
                              whole_word=whole_word, continuation=self._continuation() if whole_word else None,
                              word_clump=hp.get("word_clump", 2.0))
        return PerceiverMLM(encoder, decoder, masking)

    def _continuation(self):
        """The continuation table of ``tokenizer_path`` (default: the packaged tokenizer of the
        vocabulary size, the file the data module installs)."""
        from .data.imdb import shipped_tokenizer
        from .utils.tokenizer import continuation_table

        hp = self.hparams
        path = hp.get("tokenizer_path") or shipped_tokenizer(hp.vocab_size)
        if not os.path.exists(path):
            raise FileNotFoundError(f"whole_word_masking needs the tokenizer JSON: {path} does not exist "
                                    "(pass tokenizer_path=, the file the data was tokenized with)")
        table = continuation_table(path)
        if table.numel() != hp.vocab_size:
            raise ValueError(f"{path} has {table.numel()} tokens, vocab_size is {hp.vocab_size}: whole-word masking "
                             "needs the tokenizer of the model's vocabulary")
        return table

    def forward(self, batch):
        _, x, x_mask = batch
        return self.model(x, x_mask)

    def step(self, batch):
        _, x, x_mask = batch
        return self.model.loss(x, x_mask)

    def graph_batch(self, batch):
        return bucket_text_batch(batch, self.hparams.max_seq_len)

    def training_step(self, batch, batch_idx):
        loss = self.step(batch)
        self.log("train_loss", loss)
        return loss

    def validation_step(self, batch, batch_idx):
        self.log("val_loss", self.step(batch), prog_bar=True)

    def test_step(self, batch, batch_idx):
        self.log("test_loss", self.step(batch))

    def on_validation_epoch_end(self) -> None:
        if not self.hparams.get("masked_samples"):
            return
        trainer = self.trainer
        dm = getattr(trainer, "datamodule", None) if trainer is not None else None
        if dm is None or getattr(dm, "collator", None) is None:
            return
        samples = [s.replace("<MASK>", "[MASK]") for s in self.hparams.masked_samples]
        preds = predict_masked_samples(masked_samples=samples, encode_fn=dm.collator.encode, tokenizer=dm.tokenizer,
                                       model=self.model, device=self.device,
                                       num_predictions=self.hparams.num_predictions)
        text = "\n\n".join(["  \n".join([s] + ps) for s, ps in zip(samples, preds)])
        if self.logger is not None:
            self.logger.add_text("sample predictions", text, trainer.global_step)
