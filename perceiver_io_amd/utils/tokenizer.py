"""WordPiece tokenizer helpers (host-side data prep).

Parity: reference ``perceiver/tokenizer.py:1-40`` — same special tokens/ids
(PAD=0, UNK=1, MASK=2), same normalizer chain (extra normalizers, then
NFD → Lowercase → StripAccents), Whitespace pre-tokenizer and WordPiece
decoder, and the same JSON on-disk format (HF ``tokenizers``).  Tokenization
is CPU work feeding the GPU step; it is not a kernel target.
"""
from __future__ import annotations

from typing import Iterable

PAD_TOKEN = "[PAD]"
PAD_TOKEN_ID = 0
UNK_TOKEN = "[UNK]"
UNK_TOKEN_ID = 1
MASK_TOKEN = "[MASK]"
MASK_TOKEN_ID = 2

SPECIAL_TOKENS = [PAD_TOKEN, UNK_TOKEN, MASK_TOKEN]


def _tk():
    import tokenizers  # imported lazily: only the data path needs it

    return tokenizers


def create_tokenizer(*normalizers):
    tk = _tk()
    from tokenizers.models import WordPiece
    from tokenizers.normalizers import NFD, Lowercase, StripAccents, Sequence
    from tokenizers.pre_tokenizers import Whitespace

    tok = tk.Tokenizer(WordPiece(unk_token=UNK_TOKEN))
    tok.normalizer = Sequence(list(normalizers) + [NFD(), Lowercase(), StripAccents()])
    tok.pre_tokenizer = Whitespace()
    tok.decoder = tk.decoders.WordPiece()
    return tok


def train_tokenizer(tokenizer, data: Iterable[str], vocab_size: int):
    from tokenizers.trainers import WordPieceTrainer

    tokenizer.train_from_iterator(data, WordPieceTrainer(vocab_size=vocab_size, special_tokens=SPECIAL_TOKENS))


def save_tokenizer(tokenizer, path: str):
    tokenizer.save(path)


def load_tokenizer(path: str):
    return _tk().Tokenizer.from_file(path)


# ---- whole-word masking: which vocabulary entries continue a word -----------------------------
def continuation_table(tokenizer_or_json_path):
    """bool ``(V,)``: True where the vocabulary entry is a WordPiece continuation piece (carries
    the model's ``continuing_subword_prefix``, ``##`` by default).  Takes the path of a tokenizer
    JSON (read with plain ``json``: no ``tokenizers`` package needed) or a loaded
    ``tokenizers.Tokenizer`` (through its ``to_str()``).  ``V`` is the largest id + 1."""
    import json

    import torch

    if isinstance(tokenizer_or_json_path, (str, bytes)) or hasattr(tokenizer_or_json_path, "__fspath__"):
        with open(tokenizer_or_json_path, encoding="utf-8") as f:
            spec = json.load(f)
    else:
        spec = json.loads(tokenizer_or_json_path.to_str())
    model = spec.get("model") or {}
    vocab = model.get("vocab")
    if model.get("type", "WordPiece") != "WordPiece" or not isinstance(vocab, dict) or not vocab:
        raise ValueError("continuation_table needs a WordPiece tokenizer with a vocabulary")
    prefix = model.get("continuing_subword_prefix") or "##"
    table = torch.zeros(max(vocab.values()) + 1, dtype=torch.bool)
    for token, i in vocab.items():
        if token.startswith(prefix) and len(token) > len(prefix):
            table[i] = True
    return table


def pack_bits(table):
    """A bool ``(V,)`` table as int32 ``(⌈V / 32⌉,)``: entry ``i`` is bit ``i % 32`` of word
    ``i // 32`` (the layout the masking kernel reads)."""
    import torch

    t = table.reshape(-1).to(torch.int64)
    t = torch.nn.functional.pad(t, (0, -t.numel() % 32)).view(-1, 32)
    words = (t << torch.arange(32, dtype=torch.int64, device=t.device)).sum(1)
    return torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)


def word_clump(ids, pad, table, unk) -> float:
    """Σ len² / Σ len over the words of a ``(B, L)`` batch: the factor by which selecting whole
    words inflates the variance of the number of selected tokens over the binomial ``n·p·(1 − p)``
    (``ops.mlm_head.capacity(..., clump=)``).  The words are those of the masking kernel: the
    non-special tokens (not ``unk``, not padded) that share a word beginning, with ``table`` the
    bool ``(V,)`` continuation table; special tokens are never selected and do not count.  1.0 for
    a batch of one-token words or without any non-special token."""
    import torch

    from ..ops.emulation import word_heads

    special = ids == unk
    if pad is not None:
        special = special | pad.to(torch.bool)
    table = table.to(ids.device)
    ok = (ids >= 0) & (ids < table.numel())
    cont = ok & table[torch.where(ok, ids, torch.zeros_like(ids))]
    heads = word_heads(special, cont)[~special]
    if heads.numel() == 0:
        return 1.0
    lens = torch.unique(heads, return_counts=True)[1].to(torch.float64)
    return float((lens * lens).sum() / lens.sum())
