"""The fused text input pass (ops.fused TEXT_KV_FUSED) on the kernels' emulation: the emulated
text_kv_fwd / text_kv_bwd against embed_fwd + one ln_linear_fwd / ln_linear_bwd per layer, and
the executor's bookkeeping (pre-filled KVSource entries, one backward for both layers)."""
import pytest
import torch

from perceiver_io_amd import ops
from perceiver_io_amd.models import PerceiverDecoder, PerceiverEncoder, PerceiverMLM, TextInputAdapter, TextMasking, \
    TextOutputAdapter
from perceiver_io_amd.ops import emulation as emu

C, V, EPS = 64, 50, 1e-5
SHAPES = [(3, 40), (2, 64), (1, 7)]


def _layer(g):
    return [1 + 0.3 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g),
            (0.2 * torch.randn(2 * C, C, generator=g)).to(torch.bfloat16), 0.1 * torch.randn(2 * C, generator=g)]


def _inputs(B, L, seed=0):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, V, (B, L), generator=g)
    E = 0.1 * torch.randn(V, C, generator=g)
    P = 0.1 * torch.randn(L, C, generator=g)
    return g, ids, E, P, _layer(g), _layer(g)


@pytest.mark.parametrize("B,L", SHAPES)
def test_emulated_forward_is_the_two_launch_path(B, L):
    g, ids, E, P, la, lb = _inputs(B, L)
    x, mean, rstd, kva, kvb = emu.text_kv_fwd(ids, E, P, 8.0, EPS, la, lb)
    x0 = emu.embed_fwd(ids, E, P, 8.0)
    assert torch.equal(x, x0)
    for l, kv in ((la, kva), (lb, kvb)):
        kv0, m0, r0 = emu.ln_linear_fwd(x0.reshape(-1, C), l[0], l[1], EPS, l[2], l[3], 0, None, True, True)
        assert torch.equal(kv, kv0) and torch.equal(mean, m0) and torch.equal(rstd, r0)


@pytest.mark.parametrize("slab", [True, False])
@pytest.mark.parametrize("B,L", SHAPES)
def test_emulated_backward_matches_two_launches(B, L, slab):
    g, ids, E, P, la, lb = _inputs(B, L, 1)
    R = B * L
    x, mean, rstd, _, _ = emu.text_kv_fwd(ids, E, P, 8.0, EPS, la, lb)
    ga, gb = torch.randn(R, 2 * C, generator=g), torch.randn(R, 2 * C, generator=g)
    sizes = [C, C, 2 * C * C, 2 * C]
    rows = (R + 63) // 64 if slab else 1

    def targets():
        return [torch.zeros(rows, n) if slab else torch.zeros(n) for n in sizes]

    new = targets() + targets()
    dx = emu.text_kv_bwd(ga, gb, x, mean, rstd, la[:3], lb[:3], new, slab=slab)
    old_a, old_b = targets(), targets()
    x2 = x.reshape(R, C)
    d1 = emu.ln_linear_bwd(ga, la[2], x2, mean, rstd, la[0], la[1], None, True, *old_a, slab=slab)
    d2 = emu.ln_linear_bwd(gb, lb[2], x2, mean, rstd, lb[0], lb[1], d1, True, *old_b, slab=slab)
    for t_new, t_old in zip(new, old_a + old_b):
        assert torch.equal(t_new, t_old)
    # the only new rounding is the fp32 add before the shared LayerNorm backward
    assert (dx - d2).abs().max() <= 1e-5 * d2.abs().max()


def _mlm(layers=2, n=8, L=40):
    enc = PerceiverEncoder(TextInputAdapter(V, L, C), (n, C), layers, num_self_attention_layers_per_block=1)
    dec = PerceiverDecoder(TextOutputAdapter(V, L, C), (n, C))
    return PerceiverMLM(enc, dec, TextMasking(V))


def _encoder_grads(enc, ids, pad, w):
    enc.zero_grad()
    out = ops.fused.encoder_forward(enc, ids, pad)
    (out * w).sum().backward()
    return out.detach(), {n: p.grad.clone() for n, p in enc.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("layers", [2, 3])
def test_encoder_fused_on_matches_off(layers, monkeypatch):
    """layers = 3: layer_n applied twice, its dK|dV accumulated before the shared backward."""
    torch.manual_seed(5)
    m = _mlm(layers)
    enc = m.encoder
    ids = torch.randint(3, V, (2, 40))
    pad = torch.zeros(2, 40, dtype=torch.bool)
    pad[1, 30:] = True
    w = torch.randn(2, 8, C)
    calls = []
    real = emu.text_kv_bwd
    monkeypatch.setattr(emu, "text_kv_bwd", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    monkeypatch.setattr(ops.fused, "TEXT_KV_FUSED", True)
    out_on, g_on = _encoder_grads(enc, ids, pad, w)
    assert len(calls) == 1
    monkeypatch.setattr(ops.fused, "TEXT_KV_FUSED", False)
    out_off, g_off = _encoder_grads(enc, ids, pad, w)
    assert len(calls) == 1
    assert torch.equal(out_on, out_off)
    assert g_on.keys() == g_off.keys()
    for n, g in g_off.items():
        assert (g_on[n] - g).abs().max() <= 1e-5 * g.abs().max() + 1e-7, n


def test_frozen_layer_n_norm(monkeypatch):
    torch.manual_seed(6)
    enc = _mlm().encoder
    kvn = enc.layer_n[0][0].module.kv_norm
    kvn.weight.requires_grad_(False)
    ids = torch.randint(3, V, (2, 40))
    w = torch.randn(2, 8, C)
    monkeypatch.setattr(ops.fused, "TEXT_KV_FUSED", True)
    _, g_on = _encoder_grads(enc, ids, None, w)
    monkeypatch.setattr(ops.fused, "TEXT_KV_FUSED", False)
    _, g_off = _encoder_grads(enc, ids, None, w)
    assert kvn.weight.grad is None and g_on.keys() == g_off.keys()
    for n, g in g_off.items():
        assert (g_on[n] - g).abs().max() <= 1e-5 * g.abs().max() + 1e-7, n


def test_paths_that_keep_the_per_layer_kernels(monkeypatch):
    monkeypatch.setattr(ops.fused, "TEXT_KV_FUSED", True)
    ids = torch.randint(3, V, (2, 40))
    enc = _mlm(layers=1).encoder
    assert ops.fused._text_kv_layers(enc, enc.input_adapter, ids) is None
    enc = _mlm().encoder
    assert ops.fused._text_kv_layers(enc, enc.input_adapter, ids) is not None
    monkeypatch.setattr(ops.fused, "WGRAD_SLAB", False)
    assert ops.fused._text_kv_layers(enc, enc.input_adapter, ids) is None
