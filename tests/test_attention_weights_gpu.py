"""Head-averaged attention weights on the GPU: the ``attn_weights`` kernel (csrc/attn_weights.hip)
against its emulation on the same bf16 operands and the same ``attn_fwd`` LSE, and the recorder on
a layer that runs through its modules on the GPU against the eager fp32 ``torch`` backend."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"


def close(a, b, rel=2e-2, name=""):
    """tests/test_kernels_gpu.py ``close``: relative Frobenius error ≤ min(rel, 1 %) and max-abs
    error ≤ rel × the reference's largest value; identical non-finite patterns."""
    a, b = a.float().cpu(), b.float().cpu()
    assert a.shape == b.shape, (name, a.shape, b.shape)
    fin = torch.isfinite(b)
    assert torch.equal(torch.isfinite(a), fin), f"{name}: non-finite pattern differs"
    a, b = a[fin], b[fin]
    if b.numel() == 0:
        return
    fro = ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()
    scale = b.abs().max().item() + 1e-6
    err = (a - b).abs().max().item()
    print(f"{name}: rel fro {fro:.3e}, max err {err:.3e} (scale {scale:.3e})")
    assert fro <= min(rel, 1e-2), f"{name}: relative Frobenius error {fro:.3e}"
    assert err <= rel * scale, f"{name}: max err {err:.3e} vs scale {scale:.3e}"


# (B, Bq, H, Nq, Nk, D, packed K|V view, mask)
SHAPES = [
    (2, 2, 4, 32, 64, 16, False, None),      # exact tiles
    (1, 1, 1, 1, 1, 32, False, None),        # degenerate
    (3, 1, 4, 33, 65, 16, True, None),       # ragged both ways, broadcast queries, K a [:, :, :C] view of packed K|V
    (2, 2, 8, 64, 200, 32, False, "dead"),   # one fully padded sample, one padded from key 70
    (2, 2, 2, 300, 130, 64, False, None),    # several query tiles: the fixed-order mass reduction
    (1, 1, 1, 16, 1000, 128, False, None),   # many key tiles
]


@pytest.mark.parametrize("B,Bq,H,Nq,Nk,D,packed,mask", SHAPES)
def test_attn_weights_kernel(B, Bq, H, Nq, Nk, D, packed, mask):
    from perceiver_io_amd.ops import emulation, ext
    from perceiver_io_amd.ops.attention import pick_splits

    K = ext.require()
    torch.manual_seed(B * 1000 + Nq + Nk + D)
    C = H * D
    scale = D ** -0.5
    q = torch.randn(Bq, Nq, C, device=DEV).to(torch.bfloat16)
    kv = torch.randn(B, Nk, 2 * C if packed else C, device=DEV).to(torch.bfloat16)
    k = kv[:, :, :C]
    km = None
    if mask == "dead":
        km = torch.zeros(B, Nk, dtype=torch.bool, device=DEV)
        km[0] = True
        km[1, 70:] = True
    _, lse = K.attn_fwd(q, k, k, km, H, D, scale, 0.0, None, pick_splits(B, H, Nq, Nk))
    if km is not None:  # the forward's sentinel for a row without keys
        assert torch.isinf(lse[0]).all() and torch.isfinite(lse[1]).all()
    avg, mass = K.attn_weights(q, k, km, lse, H, D, scale, True, True)
    avg2, mass2 = K.attn_weights(q, k, km, lse, H, D, scale, True, True)
    none, mass_only = K.attn_weights(q, k, km, lse, H, D, scale, False, True)
    avg_only, none2 = K.attn_weights(q, k, km, lse, H, D, scale, True, False)
    torch.cuda.synchronize()
    assert none is None and none2 is None
    assert avg.shape == (B, Nq, Nk) and mass.shape == (B, Nk) and avg.dtype == mass.dtype == torch.float32
    e_avg, e_mass = emulation.attn_weights(q, k, km, lse, H, D, scale, True, True)
    close(avg, e_avg, 1e-3, "avg")
    close(mass, e_mass, 1e-3, "mass")
    # two launches, and the single-output instantiations, bit for bit
    assert torch.equal(avg, avg2) and torch.equal(mass, mass2)
    assert torch.equal(mass_only, mass) and torch.equal(avg_only, avg)
    if km is not None:
        assert (avg[km[:, None, :].expand_as(avg)] == 0).all() and (mass[km] == 0).all()
        assert (avg[0] == 0).all() and (mass[0] == 0).all()  # dead rows
        # whatever the dead rows' LSE holds, their keys are all padded
        l2 = lse.clone()
        l2[0] = float("nan")
        l2[0, ::2] = -3.0
        avg3, mass3 = K.attn_weights(q, k, km, l2, H, D, scale, True, True)
        assert torch.equal(avg3, avg) and torch.equal(mass3, mass)
    # the forward's LSE closes the rows: the D = 16 forward sums bf16-rounded probabilities, so
    # within 2^-9, the others within fp32 rounding of the sum
    live = torch.ones(B, Nq, device=DEV) if km is None else (~km).any(1).float()[:, None].expand(B, Nq)
    assert (avg.sum(-1) - live).abs().max().item() <= 2 ** -9 + 1e-4
    # the public ops: the same kernels behind them
    from perceiver_io_amd import ops

    with ops.backend("hip"):
        w = ops.attention_weights(q, k.contiguous(), H, km)
        m = ops.attention_mass(q, k.contiguous(), H, km)
    close(w, e_avg, 1e-3, "ops.attention_weights")
    close(m, e_mass, 1e-3, "ops.attention_mass")


def test_recorder_on_an_unfused_layer_uses_the_kernels():
    """A cross-attention layer the fused executor does not take (256 channels) runs through its
    modules on the GPU: the recorder's weights come from attn_fwd + attn_weights there, and agree
    with the eager fp32 ``torch`` backend at the bound the fused-vs-eager model tests use."""
    from perceiver_io_amd import ops
    from perceiver_io_amd.models.blocks import cross_attention_layer

    torch.manual_seed(5)
    layer = cross_attention_layer(256, 40, 4, 0.0).cuda().eval()
    xq, xkv = torch.randn(3, 37, 256, device=DEV), torch.randn(3, 70, 40, device=DEV)
    pad = torch.zeros(3, 70, dtype=torch.bool, device=DEV)
    pad[1, 50:] = True
    got = {}
    for backend in ("hip", "torch"):
        for what in ("weights", "mass"):
            with torch.no_grad(), ops.backend(backend), ops.record_attention(layer, what) as rec:
                out = layer(xq, xkv, pad)
            assert [(e["name"], e["call"]) for e in rec.entries] == [("", 0)]
            got[backend, what] = rec.entries[0]["tensor"]
        got[backend, "out"] = out
    torch.cuda.synchronize()
    assert got["hip", "weights"].shape == (3, 37, 70) and got["hip", "mass"].shape == (3, 70)
    close(got["hip", "weights"], got["torch", "weights"], name="weights")
    close(got["hip", "mass"], got["torch", "mass"], name="mass")
    close(got["hip", "out"], got["torch", "out"], name="layer output")
    assert (got["hip", "weights"][1, :, 50:] == 0).all() and (got["hip", "mass"][1, 50:] == 0).all()
