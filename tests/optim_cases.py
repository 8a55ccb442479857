"""What the flat-space optimizer tests on the GPU share (a plain module, no fixtures): the ``close``
comparison and one flat buffer of awkward tensor sizes."""
import torch

# tails of 1–3 elements, a one-chunk tensor, a chunk boundary (4096) and a multi-chunk tensor
NUMELS = [1, 3, 5, 63, 64, 65, 4095, 4096, 4097, 8193]


def close(a, b, rel, name=""):
    """tests/test_kernels_gpu.py ``close`` (the AdamW kernel check runs it with rel = 1e-5):
    relative Frobenius error and max-abs error against the reference's largest value."""
    a, b = a.float().cpu(), b.float().cpu()
    assert a.shape == b.shape, (name, a.shape, b.shape)
    fin = torch.isfinite(b)
    assert torch.equal(torch.isfinite(a), fin), f"{name}: non-finite pattern differs"
    a, b = a[fin], b[fin]
    fro = ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()
    scale = b.abs().max().item() + 1e-6
    err = (a - b).abs().max().item()
    print(f"{name}: rel fro {fro:.3e}, max err {err:.3e} (scale {scale:.3e})")
    assert fro <= min(rel, 1e-2), f"{name}: relative Frobenius error {fro:.3e}"
    assert err <= rel * scale, f"{name}: max err {err:.3e} vs scale {scale:.3e}"


def flat_case(dev="cuda"):
    """One flat buffer of the tensor sizes above (64-element alignment), built on the CPU from a
    seeded generator; the padding of m and v is NaN, that of p and g zero."""
    from perceiver_io_amd.ops.optim import ALIGN, lamb_tables

    offsets, off = [], 0
    for n in NUMELS:
        offsets.append(off)
        off += (n + ALIGN - 1) // ALIGN * ALIGN
    g = torch.Generator().manual_seed(23)
    valid = torch.zeros(off, dtype=torch.bool)
    for o, n in zip(offsets, NUMELS):
        valid[o:o + n] = True
    zero, nan = torch.zeros(off), torch.full((off,), float("nan"))
    p = torch.where(valid, torch.randn(off, generator=g), zero)
    grad = torch.where(valid, torch.randn(off, generator=g), zero)
    m = torch.where(valid, torch.randn(off, generator=g) * 0.1, nan)
    v = torch.where(valid, torch.rand(off, generator=g) * 0.01, nan)
    T = len(NUMELS)
    chunk_tab, tensor_tab, tensor_opt = lamb_tables(offsets, NUMELS, [0.01, 0.0] * (T // 2), [True, False] * (T // 2), dev)
    assert chunk_tab.shape[0] > T and off % 4 == 0
    return dict(offsets=offsets, valid=valid.to(dev), p=p.to(dev), g=grad.to(dev), m=m.to(dev), v=v.to(dev),
                chunk_tab=chunk_tab, tensor_tab=tensor_tab, tensor_opt=tensor_opt)
