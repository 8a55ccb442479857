"""Multi-head attention core: eager oracle and the HIP flash kernel.

Semantics (``nn.MultiheadAttention`` as used at reference ``perceiver/model.py:59-74``,
SURVEY App. A.2): ``softmax((q·d^-½)·kᵀ + mask)`` with ``-inf`` at padded keys,
dropout on the probabilities (training), ``P·v``, heads merged.  A query row whose keys
are *all* padded yields 0 here (the reference yields NaN; defect D10 defined).
"""
from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn.functional as F

from . import ext


def _split(x, h):
    b, n, e = x.shape
    return x.reshape(b, n, h, e // h).transpose(1, 2)


def mha_core(q, k, v, num_heads: int, key_padding_mask=None, attn_mask=None, dropout_p: float = 0.0):
    """Eager attention core on projected ``q (B, Nq, E)``, ``k, v (B, Nk, E)`` → ``(B, Nq, E)``."""
    if q.is_cuda and attn_mask is None and _hip_ok(q, num_heads):
        from . import use_hip

        if use_hip(q):
            return flash_attention(q, k, v, num_heads, key_padding_mask, dropout_p)
    b, nq, e = q.shape
    d = e // num_heads
    qh, kh, vh = _split(q, num_heads), _split(k, num_heads), _split(v, num_heads)
    s = torch.matmul(qh * (1.0 / math.sqrt(d)), kh.transpose(-1, -2))
    if attn_mask is not None:
        am = attn_mask
        if am.dtype == torch.bool:
            am = torch.zeros_like(am, dtype=s.dtype).masked_fill(am, float("-inf"))
        s = s + am
    dead = None
    if key_padding_mask is not None:
        kpm = key_padding_mask.view(b, 1, 1, -1)
        s = s.masked_fill(kpm, float("-inf"))
        dead = kpm.all(dim=-1, keepdim=True)
    p = torch.softmax(s, dim=-1)
    if dead is not None:
        p = p.masked_fill(dead, 0.0)
    if dropout_p > 0.0:
        p = F.dropout(p, p=dropout_p, training=True)
    o = torch.matmul(p, vh)
    return o.transpose(1, 2).reshape(b, nq, e)


def _weights_torch(q, k, num_heads: int, key_padding_mask=None, attn_mask=None):
    """``mha_core``'s probabilities averaged over the heads, ``(B, Nq, Nk)`` fp32 (pre-dropout)."""
    b = max(q.shape[0], k.shape[0])
    d = q.shape[-1] // num_heads
    qh, kh = _split(q.float().expand(b, -1, -1), num_heads), _split(k.float(), num_heads)
    s = torch.matmul(qh * (1.0 / math.sqrt(d)), kh.transpose(-1, -2))
    if attn_mask is not None:
        am = attn_mask
        if am.dtype == torch.bool:
            am = torch.zeros_like(am, dtype=s.dtype).masked_fill(am, float("-inf"))
        s = s + am
    if key_padding_mask is not None:
        kpm = key_padding_mask.to(torch.bool).view(b, 1, 1, -1)
        s = s.masked_fill(kpm, float("-inf"))
    p = torch.softmax(s, dim=-1)
    if key_padding_mask is not None:
        p = p.masked_fill(kpm, 0.0)  # a row whose keys are all padded: zeros, not NaN (defect D10)
    return p.sum(1) * (1.0 / num_heads)


def _weights(q, k, num_heads: int, key_padding_mask, want_avg: bool, want_mass: bool, attn_mask=None):
    """(avg | None, mass | None) on projected ``q (B|1, Nq, E)``, ``k (B, Nk, E)``, under ``no_grad``.
    HIP path: the LSE comes from the forward kernel (``v := k``, output discarded), then one
    ``attn_weights`` pass; elsewhere ``mha_core``'s math, which materialises the per-head softmax.

    Called from the recorder's hook in ``MultiHeadAttention.forward`` the HIP path runs ``attn_fwd``
    twice on the same q and k: once here for the LSE and once in ``mha_core`` for the layer's output
    (a hook next to the layer's own ``attn_fwd``, which holds that LSE already, would not)."""
    with torch.no_grad():
        if q.is_cuda and attn_mask is None and _hip_ok(q, num_heads):
            from . import use_hip

            if use_hip(q):
                d = q.shape[-1] // num_heads
                scale = 1.0 / math.sqrt(d)
                km = key_padding_mask.to(torch.bool).contiguous() if key_padding_mask is not None else None
                qb, kb = q.to(torch.bfloat16), k.to(torch.bfloat16)
                nsplit = pick_splits(k.shape[0], num_heads, q.shape[1], k.shape[1])
                _, lse = ext.attn_fwd(qb, kb, kb, km, num_heads, d, scale, 0.0, None, nsplit)
                return tuple(ext.attn_weights(qb, kb, km, lse, num_heads, d, scale, want_avg, want_mass))
        avg = _weights_torch(q, k, num_heads, key_padding_mask, attn_mask)
        return (avg if want_avg else None), (avg.sum(1) if want_mass else None)


def attention_weights(q, k, num_heads: int, key_padding_mask=None):
    """Head-averaged attention probabilities ``(B, Nq, Nk)`` fp32 of projected ``q (B|1, Nq, E)`` and
    ``k (B, Nk, E)``: ``nn.MultiheadAttention``'s ``need_weights=True`` result, before dropout.  A
    padded key has weight exactly 0; a row whose keys are all padded is all zeros.  No
    ``(B, H, Nq, Nk)`` tensor is formed on the HIP path."""
    return _weights(q, k, num_heads, key_padding_mask, True, False)[0]


def attention_mass(q, k, num_heads: int, key_padding_mask=None):
    """``attention_weights(...).sum(1)``, ``(B, Nk)`` fp32: the attention each key receives, summed
    over the queries.  On the HIP path nothing of size ``Nq·Nk`` is written."""
    return _weights(q, k, num_heads, key_padding_mask, False, True)[1]


# the open record_attention context (None outside one: the hook in MultiHeadAttention.forward costs
# one comparison)
_RECORDER = None


class AttentionRecorder:
    """What :func:`record_attention` yields: ``entries`` is a list of ``{"name", "call", "tensor"}``
    in execution order, one per cross-attention application."""

    def __init__(self, model, what: str):
        from ..models.blocks import CrossAttentionLayer

        if what not in ("mass", "weights"):
            raise ValueError(f"record_attention: what must be 'mass' or 'weights', got {what!r}")
        self.what = what
        self.entries = []
        self._layers = [(n, m) for n, m in model.named_modules() if isinstance(m, CrossAttentionLayer)]
        self._calls = {}
        self._cur = None
        self._handles = []

    @property
    def want_avg(self) -> bool:
        return self.what == "weights"

    @property
    def active(self) -> bool:
        return self._cur is not None

    def add(self, avg=None, mass=None):
        """Called by the attention of the layer in scope with whichever of the two it has."""
        if self._cur is None:
            return
        name, call = self._cur[:2]
        if self.what == "weights":
            t = avg
        else:
            t = mass if mass is not None else avg.sum(1)
        self.entries.append({"name": name, "call": call, "tensor": t.detach()})

    # module hooks on the recorded layers: installed while the context is open, so nothing of the
    # recorder exists on a layer outside it
    def _install(self):
        for name, layer in self._layers:
            self._handles.append(layer.register_forward_pre_hook(lambda m, args, name=name: self._enter(name, m)))
            self._handles.append(layer.register_forward_hook(lambda m, args, out, name=name: self._leave(name)))

    def _remove(self):
        for h in self._handles:
            h.remove()
        self._handles = []
        self._cur = None

    def _enter(self, name, layer):
        if torch.is_grad_enabled():
            raise RuntimeError(f"record_attention: {name} runs with gradients enabled; record under torch.no_grad()")
        if layer.training and layer.attn.attention.attention.dropout > 0:
            raise RuntimeError(f"record_attention: {name} runs with attention dropout active; call model.eval()")
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"record_attention: {name} runs during graph capture")
        call = self._calls.get(name, 0)
        self._calls[name] = call + 1
        self._cur = (name, call, len(self.entries))

    def _leave(self, name):
        cur, self._cur = self._cur, None
        if cur is not None and cur[0] == name and len(self.entries) == cur[2]:
            raise RuntimeError(f"record_attention: {name} ran as one fused layer, which is not recorded; run the model "
                               "on the eager backend (ops.backend('torch'))")


class record_attention:
    """Context manager: while it is open, every ``CrossAttentionLayer`` of ``model`` that runs appends
    ``{"name", "call", "tensor"}`` to ``rec.entries`` in execution order — ``name`` as in
    ``model.named_modules()``, ``call`` the application count of that module (the weight-shared
    ``layer_n`` appears ``num_layers − 1`` times), ``tensor`` the head-averaged pre-dropout weights
    ``(B, Nq, Nk)`` (``what="weights"``) or their sum over the queries ``(B, Nk)`` (``what="mass"``),
    fp32.  Self-attention layers are not recorded.  Inference only: a recorded layer raises
    ``RuntimeError`` with gradients enabled, with attention dropout active or during graph capture.

    Recorded are the layers that run through their modules (``MultiHeadAttention.forward``) only:

    * the ``torch`` and ``reference`` backends, everywhere — the weights come from the materialised
      per-head softmax (``(B, H, Nq, Nk)`` floats), as in the reference;
    * on a GPU with the HIP backend, layers the fused executor does not take (channel counts outside
      32 / 64 / 128) — there the weights come from ``attn_fwd`` + ``attn_weights`` with no per-head
      tensor, at the price of a second ``attn_fwd`` per recorded layer (``_weights``).

    The fused executor is NOT recorded: a layer that runs as one fused node raises instead of
    recording nothing, and the fused encoder, which does not go through the layer modules at all,
    leaves no entry (the model entry points built on this context refuse it up front).  Outside the
    context nothing changes."""

    def __init__(self, model, what: str = "mass"):
        self.rec = AttentionRecorder(model, what)

    def __enter__(self) -> AttentionRecorder:
        global _RECORDER
        if _RECORDER is not None:
            raise RuntimeError("record_attention: contexts do not nest")
        _RECORDER = self.rec
        self.rec._install()
        return self.rec

    def __exit__(self, *exc):
        global _RECORDER
        self.rec._remove()
        _RECORDER = None
        return False


def _hip_ok(q, num_heads) -> bool:
    e = q.shape[-1]
    return e % num_heads == 0 and (e // num_heads) in (16, 32, 64, 128)


def pick_splits(batch: int, heads: int, nq: int, nk: int, dropout: bool = False) -> int:
    """Split-KV factor so that few-query / many-key launches still fill 256 CUs."""
    waves = max(1, min(4, (nq + 31) // 32))
    blocks = ((nq + 32 * waves - 1) // (32 * waves)) * heads * batch
    tiles = (nk + 63) // 64
    if blocks >= 512:
        # ≥ 2 workgroups per CU already: a split only adds the combine launch — except for
        # 1-2-wave workgroups (≤ 64 queries, at most one wave per SIMD) doing the dropout hash
        # per score: the text classifier's cross-attention at batch 128 ran 28.6 → 18.5 µs
        # (+ a 4.8 µs combine); without dropout (15 µs) the combine eats the gain (r6)
        return 2 if dropout and blocks * waves < 2048 and tiles >= 8 else 1
    if not dropout and blocks * waves >= 512 and tiles < 16:
        # ≥ 2 waves per CU over a short key range: the 64-latent MLM cross-attention (256 two-wave
        # workgroups, 512 keys) runs 9.3 µs unsplit against 12.0 µs split in two with its
        # combine (tools/fwd_split_sweep.py, r6)
        return 1
    want = max(1, 1024 // max(blocks, 1))
    return int(max(1, min(want, tiles // 4 if tiles >= 8 else 1)))


class _FlashAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, kmask, heads, dropout_p, seed):
        d = q.shape[-1] // heads
        scale = 1.0 / math.sqrt(d)
        b = k.shape[0]
        nsplit = pick_splits(b, heads, q.shape[1], k.shape[1], dropout_p > 0)
        qb, kb, vb = (t.to(torch.bfloat16) for t in (q, k, v))
        o, lse = ext.attn_fwd(qb, kb, vb, kmask, heads, d, scale, dropout_p, seed, nsplit)
        ctx.save_for_backward(qb, kb, vb, kmask if kmask is not None else torch.empty(0), o, lse)
        ctx.cfg = (heads, d, scale, dropout_p, seed, kmask is not None, q.dtype, q.shape[0])
        return o.to(q.dtype) if q.dtype != torch.bfloat16 else o

    @staticmethod
    def backward(ctx, do):
        qb, kb, vb, km, o, lse = ctx.saved_tensors
        heads, d, scale, p, seed, has_mask, dt, bq = ctx.cfg
        dq, dk, dv = ext.attn_bwd(qb, kb, vb, km if has_mask else None, o, do.to(torch.bfloat16).contiguous(), lse,
                                  None, heads, d, scale, p, seed, None, None, None)
        if bq == 1 and dq.shape[0] > 1:
            dq = dq.sum(0, keepdim=True)
        return dq.to(dt), dk.to(dt), dv.to(dt), None, None, None, None


def flash_attention(q, k, v, num_heads: int, key_padding_mask: Optional[torch.Tensor] = None,
                    dropout_p: float = 0.0, seed: Optional[torch.Tensor] = None):
    """HIP flash attention on ``(B|1, Nq, E)`` queries and ``(B, Nk, E)`` keys/values.

    ``seed``: 1-element int64 device tensor for the dropout masks; drawn here on the device
    (graph-safe: a fresh draw on every replay of a captured step) when not given."""
    ext.require()
    if seed is None and dropout_p > 0:
        seed = torch.randint(-(2**62), 2**62, (1,), device=q.device, dtype=torch.int64)
    km = None
    if key_padding_mask is not None:
        km = key_padding_mask.to(torch.bool).contiguous()
    return _FlashAttention.apply(q, k, v, km, num_heads, float(dropout_p), seed)
