"""Lightning-layout checkpoint I/O.

Top-level keys written: ``epoch``, ``global_step``, ``pytorch-lightning_version``,
``state_dict``, ``callbacks``, ``optimizer_states``, ``lr_schedulers``, ``hparams_name``,
``hyper_parameters`` — what PL 1.5 writes and what ``load_from_checkpoint`` /
``--trainer.resume_from_checkpoint`` read (reference ``lightning.py:144-149``,
``trainer.yaml:54``).  A run with a weight EMA (``--trainer.ema_decay``) adds ``ema_state_dict``
(the averaged tensors under their ``state_dict`` names) and ``ema`` (the schedule's options);
``state_dict`` stays the raw training weights.  Everything written is reduced to tensors and plain Python values so
every checkpoint loads with ``torch.load(..., weights_only=True)``; nothing is ever fully
unpickled.
"""
from __future__ import annotations

import os
from collections import OrderedDict
from typing import Any, Dict, Optional

import torch

PL_VERSION = "1.5.10"
TAG = "perceiver_io_amd"


def _plain(obj):
    """Tensors and plain Python containers/scalars only (safe for ``weights_only``)."""
    if isinstance(obj, torch.Tensor):
        return obj.detach().cpu()
    if isinstance(obj, dict):
        return {(k if isinstance(k, (str, int)) else str(k)): _plain(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return type(obj)(_plain(v) for v in obj)
    if isinstance(obj, (str, int, float, bool)) or obj is None:
        return obj
    return str(obj)


def parameter_names(model, params):
    """The ``state_dict`` names of ``params`` (parameters of ``model``), in their order."""
    names = {id(p): n for n, p in model.named_parameters()}
    return [names[id(p)] for p in params]


def make_checkpoint(model, epoch: int, global_step: int, optimizers=(), schedulers=(), callbacks: Optional[Dict] = None,
                    ema=None):
    """``ema`` (an ``ops.optim.WeightEMA``): ``state_dict`` stays the raw training weights, so a
    resume is exact; the averaged tensors go to ``ema_state_dict`` under the same names and the
    schedule's options to ``ema`` (see :func:`averaged_state_dict`)."""
    sd = OrderedDict((k, v.detach().cpu()) for k, v in model.state_dict().items())
    extra = {}
    if ema is not None:
        extra["ema_state_dict"] = OrderedDict(
            (n, t.cpu()) for n, t in zip(parameter_names(model, ema.params), ema.state_dict()))
        extra["ema"] = {"decay": float(ema.decay), "warmup": bool(ema.warmup), "update_every": int(ema.update_every)}
    return {
        "epoch": int(epoch),
        "global_step": int(global_step),
        "pytorch-lightning_version": PL_VERSION,
        "state_dict": sd,
        "callbacks": _plain(callbacks or {}),
        "optimizer_states": [_plain(o.state_dict()) for o in optimizers],
        "lr_schedulers": [_plain(s.state_dict()) for s in schedulers],
        "hparams_name": "kwargs",
        "hyper_parameters": _plain(dict(getattr(model, "hparams", {}) or {})),
        TAG: {"format": 1},
        **extra,
    }


def save_checkpoint(ckpt: Dict[str, Any], path: str):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    tmp = path + ".tmp"
    torch.save(ckpt, tmp)
    os.replace(tmp, path)


def load_checkpoint(path: str, map_location="cpu") -> Dict[str, Any]:
    """Safe load only (``weights_only=True``); a file that needs arbitrary unpickling is refused."""
    return torch.load(path, map_location=map_location, weights_only=True)


def averaged_state_dict(ckpt: Dict[str, Any]) -> "OrderedDict[str, torch.Tensor]":
    """``ckpt["state_dict"]`` with the averaged tensors of ``ckpt["ema_state_dict"]`` substituted
    (the weights to evaluate or export; buffers and frozen parameters are not averaged and stay)."""
    if "ema_state_dict" not in ckpt:
        raise KeyError("the checkpoint holds no ema_state_dict (it was written without a weight EMA)")
    sd = OrderedDict(ckpt["state_dict"])
    for k, v in ckpt["ema_state_dict"].items():
        if k not in sd:
            raise KeyError(f"ema_state_dict entry {k!r} has no counterpart in state_dict")
        sd[k] = v
    return sd
