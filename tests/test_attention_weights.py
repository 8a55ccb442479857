"""Head-averaged attention weights on the CPU: ``ops.attention_weights`` / ``attention_mass`` and
their emulation entry point, the ``ops.record_attention`` recorder on the eager backends, and the
model entry points ``PerceiverEncoder.input_attention``, ``PerceiverMLM.token_attention`` and
``LArPerceiver.attention_map``."""
import pytest
import torch

from perceiver_io_amd import ops
from perceiver_io_amd.data.synthetic import lartpc_event
from perceiver_io_amd.models.adapters import TextInputAdapter, TextOutputAdapter
from perceiver_io_amd.models.blocks import CrossAttention, cross_attention_layer
from perceiver_io_amd.models.lartpc import LArPerceiver
from perceiver_io_amd.models.perceiver import PerceiverDecoder, PerceiverEncoder, PerceiverMLM, TextMasking

E, H, KDIM, NQ, NK = 64, 4, 24, 5, 9


def _cross_layer(dropout=0.0):
    torch.manual_seed(0)
    return cross_attention_layer(E, KDIM, H, dropout).eval()


def _inputs(b=3):
    g = torch.Generator().manual_seed(1)
    return torch.randn(b, NQ, E, generator=g), torch.randn(b, NK, KDIM, generator=g)


def _mask(b=3, full=None):
    m = torch.zeros(b, NK, dtype=torch.bool)
    m[0, 6:] = True
    m[1, ::2] = True
    if full is not None:
        m[full] = True
    return m


def _record(model, what, backend, *args):
    with torch.no_grad(), ops.backend(backend), ops.record_attention(model, what) as rec:
        out = model(*args)
    return rec.entries, out


@pytest.mark.parametrize("masked", [False, True])
def test_backends_agree(masked):
    """The torch backend's recorded weights are torch's own need_weights=True output (what the
    reference backend keeps from F.multi_head_attention_forward)."""
    layer = _cross_layer()
    assert isinstance(layer.attn, CrossAttention)
    xq, xkv = _inputs()
    mask = _mask() if masked else None
    ours, out_t = _record(layer, "weights", "torch", xq, xkv, mask)
    ref, out_r = _record(layer, "weights", "reference", xq, xkv, mask)
    assert len(ours) == len(ref) == 1 and ours[0]["name"] == ref[0]["name"] == "" and ours[0]["call"] == 0
    assert ours[0]["tensor"].shape == (3, NQ, NK) and ours[0]["tensor"].dtype == torch.float32
    torch.testing.assert_close(ours[0]["tensor"], ref[0]["tensor"])
    torch.testing.assert_close(out_t, out_r)
    mass_t = _record(layer, "mass", "torch", xq, xkv, mask)[0][0]["tensor"]
    mass_r = _record(layer, "mass", "reference", xq, xkv, mask)[0][0]["tensor"]
    assert mass_t.shape == (3, NK)
    torch.testing.assert_close(mass_t, mass_r)


def test_invariants():
    g = torch.Generator().manual_seed(2)
    q, k = torch.randn(3, NQ, E, generator=g), torch.randn(3, NK, E, generator=g)
    mask = _mask(full=2)  # sample 2: every key padded
    w = ops.attention_weights(q, k, H, mask)
    m = ops.attention_mass(q, k, H, mask)
    assert w.shape == (3, NQ, NK) and m.shape == (3, NK) and w.dtype == m.dtype == torch.float32
    assert torch.isfinite(w).all() and torch.isfinite(m).all()
    torch.testing.assert_close(w[:2].sum(-1), torch.ones(2, NQ))
    assert (w[mask[:, None, :].expand_as(w)] == 0).all()
    assert (w[2] == 0).all() and (m[2] == 0).all()
    torch.testing.assert_close(m, w.sum(1))
    live = torch.tensor([float(NQ), float(NQ), 0.0])  # query rows with at least one valid key
    torch.testing.assert_close(m.sum(-1), live)
    # one query stream broadcast over the batch
    torch.testing.assert_close(ops.attention_weights(q[:1], k, H, mask), ops.attention_weights(q[:1].expand(3, -1, -1), k, H, mask))
    # without a mask: plain softmax rows
    torch.testing.assert_close(ops.attention_weights(q, k, H).sum(-1), torch.ones(3, NQ))


def test_emulation_entry_point():
    """emulation.attn_weights: the fp32 softmax of the given operands, or 2^(s − lse) with the
    forward's LSE — both keep rows summing to 1 within the 1e-3 the GPU test allows the kernel."""
    from perceiver_io_amd.ops import emulation

    g = torch.Generator().manual_seed(3)
    d = E // H
    q = torch.randn(3, NQ, E, generator=g).to(torch.bfloat16)
    kv = torch.randn(3, NK, 2 * E, generator=g).to(torch.bfloat16)
    k = kv[:, :, :E]  # K as a view of packed K|V rows
    mask = _mask(full=2)
    scale = d ** -0.5
    _, lse = emulation.attn_fwd(q, k, k, mask, H, d, scale, 0.0, None, 1)
    want = ops.attention_weights(q.float(), k.float(), H, mask)
    for given in (None, lse):
        avg, mass = emulation.attn_weights(q, k, mask, given, H, d, scale, True, True)
        torch.testing.assert_close(avg, want)
        torch.testing.assert_close(mass, want.sum(1))
        assert (avg[2] == 0).all() and (avg[mask[:, None, :].expand_as(avg)] == 0).all()
        assert (avg[:2].sum(-1) - 1).abs().max() <= 1e-3
    # a sentinel other than +inf in a dead row's LSE changes nothing: its keys are all padded
    for sentinel in (float("-inf"), float("nan"), 0.0):
        l2 = lse.clone()
        l2[2] = sentinel
        avg2, _ = emulation.attn_weights(q, k, mask, l2, H, d, scale, True, False)
        assert torch.equal(avg2, avg)
    assert emulation.attn_weights(q, k, mask, lse, H, d, scale, False, True)[0] is None
    with pytest.raises(ValueError):
        emulation.attn_weights(q, k, mask, lse, H, d, scale, False, False)


def _mlm(num_layers=3, dropout=0.0, vocab=50, L=12):
    torch.manual_seed(4)
    enc = PerceiverEncoder(TextInputAdapter(vocab, L, 32), (8, 32), num_layers=num_layers, dropout=dropout)
    dec = PerceiverDecoder(TextOutputAdapter(vocab, L, 32), (8, 32), dropout=dropout)
    return PerceiverMLM(enc, dec, TextMasking(vocab)).eval()


def _text(L=12, vocab=50):
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(3, vocab, (2, L), generator=g)
    pad = torch.zeros(2, L, dtype=torch.bool)
    pad[1, 7:] = True
    return ids, pad


@pytest.mark.parametrize("backend", ["torch", "reference"])
def test_recorder_order_and_names(backend):
    model = _mlm()
    ids, pad = _text()
    with torch.no_grad(), ops.backend(backend), ops.record_attention(model, "mass") as rec:
        model(ids, pad, masking=False)
    got = [(e["name"], e["call"]) for e in rec.entries]
    assert got == [("encoder.layer_1.0", 0), ("encoder.layer_n.0", 0), ("encoder.layer_n.0", 1),
                   ("decoder.cross_attention", 0)]  # no entry for the six self-attention layers
    for e in rec.entries[:3]:
        assert e["tensor"].shape == (2, 12)
        assert (e["tensor"][pad] == 0).all()
        torch.testing.assert_close(e["tensor"].sum(-1), torch.full((2,), 8.0))
    assert rec.entries[3]["tensor"].shape == (2, 8)  # the decoder's 12 queries over the 8 latents
    torch.testing.assert_close(rec.entries[3]["tensor"].sum(-1), torch.full((2,), 12.0))
    # after the context closes a forward records nothing
    with torch.no_grad(), ops.backend(backend):
        model(ids, pad, masking=False)
    assert len(rec.entries) == 4 and ops.attention._RECORDER is None


def test_recorder_weights_and_output_unchanged():
    model = _mlm()
    ids, pad = _text()
    with torch.no_grad(), ops.backend("torch"):
        before = model(ids, pad, masking=False)[0]
        with ops.record_attention(model, "weights") as rec:
            during = model(ids, pad, masking=False)[0]
        with ops.record_attention(model.encoder, "mass") as rec_m:  # names relative to the recorded module
            model(ids, pad, masking=False)
    assert torch.equal(before, during)
    assert [e["tensor"].shape for e in rec.entries] == [(2, 8, 12)] * 3 + [(2, 12, 8)]
    assert [(e["name"], e["call"]) for e in rec_m.entries] == [("layer_1.0", 0), ("layer_n.0", 0), ("layer_n.0", 1)]
    for w, m in zip(rec.entries, rec_m.entries):
        torch.testing.assert_close(w["tensor"].sum(1), m["tensor"])


def test_recorder_raises():
    ids, pad = _text()
    model = _mlm(dropout=0.1)
    with ops.backend("torch"):
        with ops.record_attention(model, "mass"):
            with pytest.raises(RuntimeError, match="gradients"):
                model(ids, pad, masking=False)
        model.train()
        with torch.no_grad(), ops.record_attention(model, "mass"):
            with pytest.raises(RuntimeError, match="dropout"):
                model(ids, pad, masking=False)
        model.eval()
        with torch.no_grad(), ops.record_attention(model, "mass") as rec:
            model(ids, pad, masking=False)
            with pytest.raises(RuntimeError, match="nest"):
                with ops.record_attention(model, "mass"):
                    pass
        assert len(rec.entries) == 4
    with pytest.raises(ValueError):
        ops.record_attention(model, "scores")
    assert ops.attention._RECORDER is None


def test_input_and_token_attention():
    model = _mlm()
    ids, pad = _text()
    with ops.backend("torch"):
        masses = model.encoder.input_attention(ids, pad)
        tok = model.token_attention(ids, pad)
    assert len(masses) == 3 and all(m.shape == (2, 12) for m in masses)
    assert torch.equal(tok, masses[0])
    assert (tok[pad] == 0).all() and (tok[~pad] > 0).all()
    torch.testing.assert_close(tok.sum(-1), torch.full((2,), 8.0))


@pytest.fixture(scope="module")
def lar_case():
    torch.manual_seed(6)
    model = LArPerceiver(32, latents=(8, 32), bands=8).eval()
    img = torch.stack([lartpc_event(20 + i, 32)[0] for i in range(2)])
    return model, img


def test_lartpc_attention_map(lar_case):
    model, img = lar_case
    flat = img.reshape(2, -1)
    lit = flat != 0
    assert lit.sum(1).min() > 8
    with ops.backend("torch"):
        amap = model.attention_map(img, bucket=16)
        last = model.attention_map(img, bucket=16, layer=2)
        with pytest.raises(ValueError):
            model.attention_map(img, bucket=16, layer=3)
    assert amap.shape == (2, 32 * 32) and amap.dtype == torch.float32
    assert (amap[~lit] == 0).all() and (amap[lit] > 0).all()
    torch.testing.assert_close(amap.sum(1), torch.full((2,), 8.0))
    torch.testing.assert_close(last.sum(1), torch.full((2,), 8.0))
    assert not torch.equal(last, amap)
    # the same mass as recording the sparse encoder by hand
    coll = ops.emulation.nonzero_compact(flat, int(lit.sum(1).max()))
    from perceiver_io_amd.models.lartpc import sparse_inputs

    with torch.no_grad(), ops.backend("torch"), ops.record_attention(model.encoder, "mass") as rec:
        model.encoder.forward_inputs(sparse_inputs(model.encoder.input_adapter, coll[0], coll[1]), coll[2])
    torch.testing.assert_close(amap.gather(1, coll[1])[~coll[2]], rec.entries[0]["tensor"][~coll[2]])


def test_lartpc_attention_map_capacity(lar_case):
    model, img = lar_case
    flat = img.reshape(2, -1)
    cap = 8
    with ops.backend("torch"):
        amap = model.attention_map(img, capacity=cap)
    lit = flat != 0
    rank = torch.cumsum(lit, 1) - 1  # flat-order rank of each lit pixel
    kept = lit & (rank < cap)
    assert (amap[~kept] == 0).all() and (amap[kept] > 0).all()
    assert (lit & ~kept).any()  # pixels past the capacity exist and are 0
    torch.testing.assert_close(amap.sum(1), torch.full((2,), 8.0))
