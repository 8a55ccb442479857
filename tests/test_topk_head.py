"""Vocabulary top-k head on the CPU: the kernel emulation (``ops.emulation.vocab_topk``), the op's
eager path (``ops.mlm_head.vocab_topk``) and the models' ``predict_topk``."""
import pytest
import torch
import torch.nn.functional as F


def _bf(x):
    return x.to(torch.bfloat16).to(torch.float32)


def _gathered_logit_check(ref_rows, values, indices, rel):
    """every returned index holds a logit as large as the true one of its rank, to ``rel`` of the
    logits' scale (any correct answer under near-ties passes, no row is left out), and the
    returned value is the logit at that index"""
    k = values.shape[1]
    bound = rel * ref_rows.abs().max().item()
    at = ref_rows.gather(1, indices)
    assert (at - ref_rows.topk(k, dim=-1).values).abs().max().item() <= bound
    assert (at - values).abs().max().item() <= bound


def test_emulation_vocab_topk_matches_topk_and_logsumexp():
    from perceiver_io_amd.ops import emulation

    torch.manual_seed(0)
    M, V, C, k = 37, 301, 64, 5
    h = _bf(torch.randn(2 * M, C))
    w = (torch.randn(V, C) * 0.3).to(torch.bfloat16)
    bias = torch.randn(V) * 0.1
    idx = torch.randperm(2 * M)[:M]
    logits = h[idx] @ w.float().t() + bias
    values, indices, lse = emulation.vocab_topk(h, idx, w, bias, k)
    tv, ti = logits.topk(k, dim=-1)
    assert values.shape == (M, k) and indices.shape == (M, k) and lse.shape == (M,)
    assert indices.dtype == torch.int64
    assert torch.equal(values, tv)
    assert torch.equal(logits.gather(1, indices), tv)
    assert torch.allclose(lse, torch.logsumexp(logits, -1), rtol=1e-6, atol=1e-6)
    # no idx: every row
    v2, i2, l2 = emulation.vocab_topk(h[idx].contiguous(), None, w, bias, k)
    assert torch.equal(v2, values) and torch.equal(i2, indices) and torch.equal(l2, lse)
    # fp32 inputs are rounded to bf16 where the kernel stages bf16 operands
    hn = torch.randn(M, C)
    v3 = emulation.vocab_topk(hn, None, w, bias, k)[0]
    assert torch.equal(v3, (_bf(hn) @ w.float().t() + bias).topk(k, dim=-1).values)


def test_emulation_vocab_topk_tie_rule():
    """two vocabulary rows with identical weights and bias: the lower index comes first"""
    from perceiver_io_amd.ops import emulation

    torch.manual_seed(1)
    V, C = 300, 64
    w = (torch.randn(V, C) * 0.3).to(torch.bfloat16)
    bias = torch.randn(V) * 0.1
    for dup in (200, 21, 18):
        w2, b2 = w.clone(), bias.clone()
        w2[dup], b2[dup] = w2[17], b2[17]
        h = _bf(8.0 * w2[17].float()[None, :] + 0.05 * torch.randn(9, C))
        logits = h @ w2.float().t() + b2
        top2 = logits.topk(2, dim=-1).values
        assert torch.equal(top2[:, 0], logits[:, 17]) and torch.equal(top2[:, 1], logits[:, dup])
        _, indices, _ = emulation.vocab_topk(h, None, w2, b2, 3)
        assert (indices[:, 0] == 17).all() and (indices[:, 1] == dup).all()


@pytest.mark.parametrize("C,k", [(64, 5), (32, 3), (128, 9)])
def test_op_vocab_topk_cpu_is_fp32_linear_topk(C, k):
    from perceiver_io_amd.ops.mlm_head import vocab_topk

    torch.manual_seed(2)
    M, V = 23, 211
    h = torch.randn(3, 11, C)  # not bf16-exact: the CPU path must not round
    weight = torch.randn(V, C) * 0.3
    bias = torch.randn(V) * 0.1
    idx = torch.randperm(33)[:M]
    logits = F.linear(h.reshape(-1, C)[idx], weight, bias)
    values, indices, lse = vocab_topk(h, weight, bias, k, idx=idx)
    tv, ti = logits.topk(k, dim=-1)
    assert torch.equal(values, tv) and torch.equal(indices, ti)
    assert torch.equal(lse, torch.logsumexp(logits, -1))
    va, ia, la = vocab_topk(h, weight, bias, k)
    full = F.linear(h.reshape(-1, C), weight, bias)
    assert torch.equal(va, full.topk(k, dim=-1).values) and la.shape == (33,)
    with pytest.raises(ValueError):
        vocab_topk(h, weight, bias, V + 1)


def _small_mlm(V=97, L=24, C=32):
    from perceiver_io_amd.models import (PerceiverDecoder, PerceiverEncoder, PerceiverMLM, TextInputAdapter,
                                         TextMasking, TextOutputAdapter)

    enc = PerceiverEncoder(TextInputAdapter(V, L, C), (8, C), 2, num_self_attention_layers_per_block=1)
    dec = PerceiverDecoder(TextOutputAdapter(V, L, C), (8, C))
    return PerceiverMLM(enc, dec, TextMasking(V)).eval()


def test_mlm_predict_topk_cpu_matches_full_logits():
    torch.manual_seed(3)
    V, L, k = 97, 24, 5
    model = _small_mlm(V, L)
    mask_id = model.masking.mask_token_id
    ids = torch.randint(3, V, (4, L))
    ids[0, [2, 9, 10, 23]] = mask_id
    ids[2, 5] = mask_id  # sequences 1 and 3 have no [MASK]
    pad = torch.zeros(4, L, dtype=torch.bool)
    pad[2, 18:] = True
    ids[2, 18:] = 0
    where, values, indices, lse = model.predict_topk(ids, pad, k=k)
    positions = ids == mask_id
    assert torch.equal(where, positions.nonzero()) and where.dtype == torch.int64
    with torch.no_grad():
        logits, labels = model(ids, pad, masking=False)
    assert labels is None
    ref = logits[positions].float()
    assert values.shape == (5, k) and indices.shape == (5, k) and lse.shape == (5,)
    tv = ref.topk(k, dim=-1).values
    assert ((values - tv).norm() / tv.norm()).item() < 1e-5
    _gathered_logit_check(ref, values, indices, 1e-5)
    assert torch.allclose(lse, torch.logsumexp(ref, -1), rtol=1e-5, atol=1e-5)
    assert not values.requires_grad
    # explicit positions: any token, not only [MASK]
    pos = torch.zeros(4, L, dtype=torch.bool)
    pos[1, 0] = pos[3, 7] = pos[3, 8] = True
    w2, v2, i2, _ = model.predict_topk(ids, pad, k=2, positions=pos)
    assert torch.equal(w2, pos.nonzero())
    _gathered_logit_check(logits[pos].float(), v2, i2, 1e-5)


def test_mlm_predict_topk_cpu_without_masks_is_empty():
    torch.manual_seed(4)
    model = _small_mlm()
    ids = torch.randint(3, 97, (3, 24))
    where, values, indices, lse = model.predict_topk(ids, None, k=4)
    assert where.shape == (0, 2) and values.shape == (0, 4) and indices.shape == (0, 4) and lse.shape == (0,)
    assert where.dtype == torch.int64 and indices.dtype == torch.int64


def test_classifier_predict_topk_cpu():
    from perceiver_io_amd.models import (ClassificationOutputAdapter, ImageInputAdapter, PerceiverDecoder,
                                         PerceiverEncoder, PerceiverIO)

    torch.manual_seed(5)
    C, classes = 32, 10
    enc = PerceiverEncoder(ImageInputAdapter((8, 8, 1), 4), (8, C), 2, num_self_attention_layers_per_block=1)
    dec = PerceiverDecoder(ClassificationOutputAdapter(classes, num_output_channels=C), (8, C))
    model = PerceiverIO(enc, dec).eval()
    x = torch.randn(6, 8, 8, 1)
    with torch.no_grad():
        logits = model(x)
    values, indices, lse = model.predict_topk(x, k=3)
    assert values.shape == (6, 3) and indices.shape == (6, 3) and lse.shape == (6,)
    assert torch.equal(indices[:, 0], logits.argmax(-1))
    assert torch.allclose(values, logits.topk(3, dim=-1).values, rtol=1e-5, atol=1e-6)
    assert torch.allclose(lse, torch.logsumexp(logits, -1), rtol=1e-5, atol=1e-6)
    v1, i1, _ = model.predict_topk(x)  # k = 1 by default
    assert i1.shape == (6, 1) and torch.equal(i1[:, 0], logits.argmax(-1))
    # a decoder with more than one output query has no single class per sample
    dec2 = PerceiverDecoder(ClassificationOutputAdapter(classes, num_outputs=3, num_output_channels=C), (8, C))
    with pytest.raises(ValueError):
        PerceiverIO(enc, dec2).eval().predict_topk(x)
