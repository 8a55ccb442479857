"""Numerics of every HIP kernel against its plain-PyTorch fp32 emulation (ops/emulation.py).

Each test feeds identical inputs to ``perceiver_io_amd._C`` and ``ops.emulation`` and
compares with tolerances scaled to the output magnitude (bf16 operands, fp32 accumulate).
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _ext():
    from perceiver_io_amd.ops import ext

    return ext.require()


def _emu():
    from perceiver_io_amd.ops import emulation

    return emulation


def close(a, b, rel=2e-2, name=""):
    """Per output: relative Frobenius error ≤ min(rel, 1 %) (sensitive to errors anywhere, also in
    small-magnitude regions) AND max-abs error ≤ rel × the reference's largest value (a local
    outlier cannot hide in the norm); identical non-finite patterns."""
    a, b = a.float().cpu(), b.float().cpu()
    assert a.shape == b.shape, (name, a.shape, b.shape)
    fin = torch.isfinite(b)
    assert torch.equal(torch.isfinite(a), fin), f"{name}: non-finite pattern differs"
    a, b = a[fin], b[fin]
    if b.numel() == 0:
        return
    fro = ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()
    assert fro <= min(rel, 1e-2), f"{name}: relative Frobenius error {fro:.3e}"
    scale = b.abs().max().item() + 1e-6
    err = (a - b).abs().max().item()
    assert err <= rel * scale, f"{name}: max err {err:.3e} vs scale {scale:.3e}"


def bf(x):
    return x.to(torch.bfloat16)


def test_cross_lane_reductions():
    x = torch.randn(64, device=DEV)
    out = _ext().reduce_probe(x).cpu()
    xc = x.cpu()
    idx = torch.arange(64)
    halves = xc.view(2, 32)
    torch.testing.assert_close(out[0], xc.sum().expand(64), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(out[1], xc.max().expand(64))
    torch.testing.assert_close(out[2], halves.sum(1).repeat_interleave(32), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(out[3], halves.max(1).values.repeat_interleave(32))
    torch.testing.assert_close(out[4], xc + xc[idx ^ 16])
    torch.testing.assert_close(out[5], xc + xc[idx ^ 32])


@pytest.mark.parametrize("R,Kin,N,xbf", [(200, 64, 192, False), (130, 131, 128, False), (64, 64, 64, True)])
def test_ln_linear_fwd(R, Kin, N, xbf):
    torch.manual_seed(0)
    x = torch.randn(R, Kin, device=DEV) * 2 + 0.5
    if xbf:
        x = bf(x)
    w = bf(torch.randn(N, Kin, device=DEV) / math.sqrt(Kin))
    lw, lb = torch.randn(Kin, device=DEV), torch.randn(Kin, device=DEV)
    b = torch.randn(N, device=DEV)
    res = torch.randn(R, N, device=DEV)
    for act, r, ob in ((0, None, True), (1, res, False)):
        y1 = _ext().ln_linear_fwd(x, lw, lb, 1e-5, w, b, act, r, ob, True)
        y2 = _emu().ln_linear_fwd(x, lw, lb, 1e-5, w, b, act, r, ob, True)
        close(y1[0], y2[0], name="y")
        close(y1[1], y2[1], 1e-4, "mean")
        close(y1[2], y2[2], 1e-3, "rstd")


def _attn_inputs(B, Bq, Nq, Nk, H, D, packed=True, mask=True):
    E = H * D
    q = bf(torch.randn(Bq, Nq, 3 * E if packed else E, device=DEV))
    kv = bf(torch.randn(B, Nk, 2 * E, device=DEV))
    qv = q[:, :, :E]
    k, v = kv[:, :, :E], kv[:, :, E:]
    km = None
    if mask:
        km = torch.rand(B, Nk, device=DEV) < 0.3
        km[0] = True  # a fully padded batch row (defect D10: defined as zero output)
    return qv, k, v, km


@pytest.mark.parametrize("B,Bq,Nq,Nk,H,D,ns", [
    (3, 3, 70, 100, 4, 16, 1),
    (2, 1, 40, 300, 4, 16, 1),
    (2, 2, 32, 1000, 4, 32, 4),
    (2, 2, 96, 64, 2, 64, 1),
    (2, 2, 33, 80, 1, 128, 2),
    # ≥ 4 key blocks per (batch, head) adding into dQ
    (2, 2, 40, 3000, 4, 16, 4),
    (2, 1, 40, 1200, 4, 16, 2),
    (2, 2, 64, 2000, 2, 64, 4),
    (2, 2, 33, 800, 1, 128, 2),
    # many queries over a few keys (decoder pixel / token queries over the latents): the query
    # range is split across workgroups, dK / dV partials added atomically
    (4, 4, 4000, 32, 1, 64, 1),
    (2, 2, 3000, 40, 4, 16, 1),
    (2, 2, 2500, 64, 2, 32, 1),
])
def test_attention_fwd_bwd(B, Bq, Nq, Nk, H, D, ns):
    torch.manual_seed(1)
    q, k, v, km = _attn_inputs(B, Bq, Nq, Nk, H, D)
    scale = 1.0 / math.sqrt(D)
    o1, l1 = _ext().attn_fwd(q, k, v, km, H, D, scale, 0.0, None, ns)
    o2, l2 = _emu().attn_fwd(q, k, v, km, H, D, scale, 0.0, None, ns)
    close(o1, o2, name="O")
    close(l1, l2, 1e-3, "lse")
    assert o1[0].abs().max().item() == 0.0  # fully masked rows → 0
    do = bf(torch.randn(B, Nq, H * D, device=DEV))
    g1 = _ext().attn_bwd(q, k, v, km, o1, do, l1, None, H, D, scale, 0.0, None, None, None, None)
    g2 = _emu().attn_bwd(q, k, v, km, o1, do, l1, None, H, D, scale, 0.0, None, None, None, None)
    for a, b, n in zip(g1, g2, ("dq", "dk", "dv")):
        close(a, b, 3e-2, n)
    # packed, uninitialised output buffer (the kernel must overwrite / clear dQ itself)
    if Bq == B:
        E = H * D
        pk = torch.full((B, Nq, 3 * E), float("nan"), device=DEV)
        dkv = torch.full((B, Nk, 2 * E), float("nan"), device=DEV)
        _ext().attn_bwd(q, k, v, km, o1, do, l1, None, H, D, scale, 0.0, None, pk[:, :, :E], dkv[:, :, :E], dkv[:, :, E:])
        close(pk[:, :, :E], g2[0], 3e-2, "dq packed")
        close(dkv[:, :, :E], g2[1], 3e-2, "dk packed")
        close(dkv[:, :, E:], g2[2], 3e-2, "dv packed")
        # K/V shared by several layers: the second application adds onto the first
        _ext().attn_bwd(q, k, v, km, o1, do, l1, None, H, D, scale, 0.0, None, pk[:, :, :E], dkv[:, :, :E], dkv[:, :, E:],
                        True)
        close(dkv[:, :, :E], 2 * g2[1], 3e-2, "dk accumulated")
        close(dkv[:, :, E:], 2 * g2[2], 3e-2, "dv accumulated")


def test_attention_bwd_deterministic_key_blocks():
    """Deterministic mode with several key blocks: each block stores its own dQ slice and the
    slices are summed in a fixed order — same values as the atomic path's reference, and bit for
    bit the same from run to run."""
    from perceiver_io_amd import ops

    torch.manual_seed(2)
    B, Nq, Nk, H, D = 2, 64, 600, 4, 16
    q, k, v, km = _attn_inputs(B, B, Nq, Nk, H, D)
    scale = 1.0 / math.sqrt(D)
    o, lse = _ext().attn_fwd(q, k, v, km, H, D, scale, 0.0, None, 1)
    do = bf(torch.randn(B, Nq, H * D, device=DEV))
    ref = _emu().attn_bwd(q, k, v, km, o, do, lse, None, H, D, scale, 0.0, None, None, None, None)
    ops.set_deterministic(True)  # put back by the autouse fixture
    runs = [_ext().attn_bwd(q, k, v, km, o, do, lse, None, H, D, scale, 0.0, None, None, None, None) for _ in range(2)]
    for a, b, n in zip(runs[0], ref, ("dq", "dk", "dv")):
        close(a, b, 3e-2, n)
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def _seed(v):
    return torch.tensor([v], dtype=torch.int64, device=DEV)


def test_attention_dropout_statistics():
    torch.manual_seed(2)
    B, Nq, Nk, H, D = 2, 64, 256, 4, 16
    q, k, v, _ = _attn_inputs(B, B, Nq, Nk, H, D, mask=False)
    v = torch.ones_like(v)
    o, _ = _ext().attn_fwd(q, k, v, None, H, D, 0.25, 0.25, _seed(123), 1)
    # E[dropout(P)·1] = 1 per row; rows average close to 1
    m = o.float().mean().item()
    assert abs(m - 1.0) < 0.05, m
    o2, _ = _ext().attn_fwd(q, k, v, None, H, D, 0.25, 0.25, _seed(123), 1)
    assert torch.equal(o, o2)  # deterministic for a given device seed
    o3, _ = _ext().attn_fwd(q, k, v, None, H, D, 0.25, 0.25, _seed(124), 1)
    assert not torch.equal(o, o3)  # a new seed draws new masks
    o4, _ = _ext().attn_fwd(q, k, v, None, H, D, 0.25, 0.25, _seed(123), 1, site=1)
    assert not torch.equal(o, o4)  # so does another call site


@pytest.mark.parametrize("B,Bq,Nq,Nk,H,D,ns,p", [
    (3, 3, 70, 200, 4, 16, 1, 0.1),
    (2, 1, 32, 900, 4, 32, 3, 0.3),
    (2, 2, 96, 64, 1, 64, 1, 0.5),
    (2, 2, 1500, 32, 1, 64, 1, 0.2),
    # head width 16 over ≤ 64 keys (the 64-latent self-attention): the two-wave backward
    (5, 5, 64, 64, 4, 16, 1, 0.1),
    (5, 5, 64, 64, 4, 16, 1, 0.0),
    (3, 3, 33, 64, 4, 16, 1, 0.1),
    (3, 3, 33, 64, 4, 16, 1, 0.0),
    (2, 2, 130, 40, 4, 16, 1, 0.1),
])
def test_attention_dropout_matches_emulation(B, Bq, Nq, Nk, H, D, ns, p):
    """The kernels' hashed masks are reproduced bit-exactly by the emulation, so fwd AND bwd
    with dropout compare against the fp32 oracle like the p = 0 path."""
    torch.manual_seed(5)
    q, k, v, km = _attn_inputs(B, Bq, Nq, Nk, H, D)
    scale = 1.0 / math.sqrt(D)
    sd = _seed(987654321987)
    o1, l1 = _ext().attn_fwd(q, k, v, km, H, D, scale, p, sd, ns, site=3)
    o2, l2 = _emu().attn_fwd(q, k, v, km, H, D, scale, p, sd, ns, site=3)
    close(o1, o2, name="O (dropout)")
    close(l1, l2, 1e-3, "lse (dropout)")
    do = bf(torch.randn(B, Nq, H * D, device=DEV))
    g1 = _ext().attn_bwd(q, k, v, km, o1, do, l1, None, H, D, scale, p, sd, None, None, None, site=3)
    g2 = _emu().attn_bwd(q, k, v, km, o1, do, l1, None, H, D, scale, p, sd, None, None, None, site=3)
    for a, b, n in zip(g1, g2, ("dq", "dk", "dv")):
        close(a, b, 3e-2, n + " (dropout)")


@pytest.mark.parametrize("C,H", [(64, 4), (128, 4), (32, 1)])
def test_post_attn_residual_dropout(C, H):
    """Residual dropout in the post-attention epilogues: fwd + bwd vs the emulation with the
    same hashed masks; p = 0 through the dropout arguments is bit-identical to no dropout."""
    torch.manual_seed(6)
    R, p = 200, 0.2
    o = bf(torch.randn(R, C, device=DEV))
    x = torch.randn(R, C, device=DEV)
    ws = [bf(torch.randn(C, C, device=DEV) / math.sqrt(C)) for _ in range(3)]
    bo, b1, b2 = (torch.randn(C, device=DEV) * 0.1 for _ in range(3))
    g2, be2 = torch.randn(C, device=DEV), torch.randn(C, device=DEV)
    sd = _seed(42)
    a = _ext().post_attn_fwd(o, x, ws[0], bo, g2, be2, 1e-5, ws[1], b1, ws[2], b2, seed=sd, site=5, p=p)
    b = _emu().post_attn_fwd(o, x, ws[0], bo, g2, be2, 1e-5, ws[1], b1, ws[2], b2, seed=sd, site=5, p=p)
    for t1, t2, n in zip(a, b, ("z", "y", "mean", "rstd", "u")):
        close(t1, t2, 2e-2, n + " (dropout)")
    a0 = _ext().post_attn_fwd(o, x, ws[0], bo, g2, be2, 1e-5, ws[1], b1, ws[2], b2, seed=sd, site=5, p=0.0)
    r0 = _ext().post_attn_fwd(o, x, ws[0], bo, g2, be2, 1e-5, ws[1], b1, ws[2], b2)
    for t1, t2 in zip(a0, r0):
        assert torch.equal(t1, t2)
    # the attention-output residual branch really drops ≈ p of its elements
    att = (a[1] - x).abs() < 1e-6
    frac = att.float().mean().item()
    assert abs(frac - p) < 0.04, frac
    z, y, m, r, u = b
    dz = torch.randn(R, C, device=DEV)
    names = ("dWo", "dbo", "dg2", "dbe2", "dW1", "db1", "dW2", "db2")
    outs = []
    for K in (_ext(), _emu()):
        grads = [torch.zeros((C, C) if n.startswith("dW") else (C,), device=DEV) for n in names]
        outs.append(tuple(K.post_attn_bwd(dz, y, m, r, u, o, ws[0], ws[1], ws[2], g2, be2, H, grads, seed=sd, site=5,
                                          p=p)) + tuple(grads))
    for i, n in enumerate(("dy", "dO", "delta") + names):
        close(outs[0][i], outs[1][i], 3e-2, n + " (dropout)")


@pytest.mark.parametrize("C,H", [(64, 4), (128, 4), (32, 1)])
def test_post_attn(C, H):
    torch.manual_seed(3)
    R = 150
    o = bf(torch.randn(R, C, device=DEV))
    x = torch.randn(R, C, device=DEV)
    ws = [bf(torch.randn(C, C, device=DEV) / math.sqrt(C)) for _ in range(3)]
    bo, b1, b2 = (torch.randn(C, device=DEV) * 0.1 for _ in range(3))
    g2, be2 = torch.randn(C, device=DEV), torch.randn(C, device=DEV)
    a = _ext().post_attn_fwd(o, x, ws[0], bo, g2, be2, 1e-5, ws[1], b1, ws[2], b2)
    b = _emu().post_attn_fwd(o, x, ws[0], bo, g2, be2, 1e-5, ws[1], b1, ws[2], b2)
    for t1, t2, n in zip(a, b, ("z", "y", "mean", "rstd", "u")):
        close(t1, t2, 2e-2, n)
    # batch-broadcast residual: x has R / 3 rows, row r adds x[r % (R / 3)]
    xs = x[: R // 3].contiguous()
    a3 = _ext().post_attn_fwd(o[: 3 * (R // 3)].contiguous(), xs, ws[0], bo, g2, be2, 1e-5, ws[1], b1, ws[2], b2)
    b3 = _emu().post_attn_fwd(o[: 3 * (R // 3)].contiguous(), xs, ws[0], bo, g2, be2, 1e-5, ws[1], b1, ws[2], b2)
    close(a3[0], b3[0], 2e-2, "z (broadcast x)")
    z, y, m, r, u = b
    dz = torch.randn(R, C, device=DEV)
    outs = []
    names = ("dWo", "dbo", "dg2", "dbe2", "dW1", "db1", "dW2", "db2")
    for K in (_ext(), _emu()):
        grads = [torch.full((C, C) if n.startswith("dW") else (C,), 0.5, device=DEV) for n in names]  # accumulate
        outs.append(tuple(K.post_attn_bwd(dz, y, m, r, u, o, ws[0], ws[1], ws[2], g2, be2, H, grads)) + tuple(grads))
    ga, gb = outs
    for i, n in enumerate(("dy", "dO", "delta") + names):
        close(ga[i], gb[i], 3e-2, n)
    # slab sink: one partial row per 64-row tile (plain stores, NaN-initialised slab), then
    # slab_reduce onto the same 0.5-initialised destinations
    sizes = [C * C if n.startswith("dW") else C for n in names]
    offs = [sum(sizes[:i]) for i in range(8)]
    slab = torch.full(((R + 63) // 64, sum(sizes)), float("nan"), device=DEV)
    views = [slab[:, o:o + n] for o, n in zip(offs, sizes)]
    outs_s = _ext().post_attn_bwd(dz, y, m, r, u, o, ws[0], ws[1], ws[2], g2, be2, H, views, slab=True)
    assert torch.isfinite(slab).all()  # every tile wrote every element of its row
    dst = [torch.full((C, C) if n.startswith("dW") else (C,), 0.5, device=DEV) for n in names]
    _ext().slab_reduce(slab, dst, offs)
    for i, n in enumerate(("dy", "dO", "delta")):
        close(outs_s[i], gb[i], 3e-2, n + " (slab)")
    for i, n in enumerate(names):
        close(dst[i], gb[3 + i], 3e-2, n + " (slab)")
    # the same reduction as a job run by the appended workgroups of the next backward kernel
    dst2 = [torch.full((C, C) if n.startswith("dW") else (C,), 0.5, device=DEV) for n in names]
    scratch = [torch.zeros_like(t) for t in dst2]
    _ext().post_attn_bwd(dz, y, m, r, u, o, ws[0], ws[1], ws[2], g2, be2, H, scratch, job_slab=slab,
                         job_dsts=[t.view(-1) for t in dst2], job_offs=offs)
    for i, n in enumerate(names):
        close(dst2[i], gb[3 + i], 3e-2, n + " (slab job)")


def test_post_attn_ln_linear_fwd():
    """The row-tile layer-boundary forward (post-attention block of layer l, then LN1 + packed QKV
    projection of layer l+1) over two 64-row tiles."""
    torch.manual_seed(5)
    R, C = 128, 64
    o = bf(torch.randn(R, C, device=DEV))
    x = torch.randn(R, C, device=DEV)
    ws = [bf(torch.randn(C, C, device=DEV) / math.sqrt(C)) for _ in range(3)]
    bo, b1, b2 = (torch.randn(C, device=DEV) * 0.1 for _ in range(3))
    g2, be2 = torch.randn(C, device=DEV), torch.randn(C, device=DEV)
    lnw, lnb = torch.randn(C, device=DEV), torch.randn(C, device=DEV)
    wq, bq = bf(torch.randn(3 * C, C, device=DEV) / math.sqrt(C)), torch.randn(3 * C, device=DEV) * 0.1
    a, b = (K.post_attn_ln_linear_fwd(o, x, ws[0], bo, g2, be2, 1e-5, ws[1], b1, ws[2], b2, lnw, lnb, wq, bq)
            for K in (_ext(), _emu()))
    for t1, t2, n in zip(a, b, ("z", "y", "mean2", "rstd2", "u", "qkv", "mean1", "rstd1")):
        close(t1, t2, 2e-2, n)


@pytest.mark.parametrize("R,N,Kin,gbf", [(300, 192, 64, False), (200, 128, 131, False), (129, 64, 64, True)])
def test_ln_linear_bwd_and_wgrad(R, N, Kin, gbf):
    torch.manual_seed(4)
    g = torch.randn(R, N, device=DEV)
    if gbf:
        g = bf(g)
    w = bf(torch.randn(N, Kin, device=DEV) / math.sqrt(Kin))
    x = torch.randn(R, Kin, device=DEV) * 1.5 + 0.2
    lw, lb = torch.randn(Kin, device=DEV), torch.randn(Kin, device=DEV)
    mean = x.mean(-1)
    rstd = torch.rsqrt(x.var(-1, unbiased=False) + 1e-5)
    dres = torch.randn(R, Kin, device=DEV)
    res = []
    for K in (_ext(), _emu()):
        dg, db = torch.zeros(Kin, device=DEV), torch.zeros(Kin, device=DEV)
        dW, dbias = torch.ones(N, Kin, device=DEV), torch.ones(N, device=DEV)  # accumulate onto existing grads
        dx = K.ln_linear_bwd(g, w, x, mean, rstd, lw, lb, dres, True, dg, db, dW, dbias)
        res.append((dx, dg, db, dW, dbias))
    for i, n in enumerate(("dx", "dgamma", "dbeta", "dW", "dbias")):
        close(res[0][i], res[1][i], 3e-2 if i < 4 else 1e-4, n)
    # slab sink (segments 4-aligned, odd Kin included) + slab_reduce
    sizes = [Kin, Kin, N * Kin, N]
    offs, P = [], 0
    for n_ in sizes:
        offs.append(P)
        P += (n_ + 3) // 4 * 4
    slab = torch.full(((R + 63) // 64, P), float("nan"), device=DEV)
    views = [slab[:, o:o + n_] for o, n_ in zip(offs, sizes)]
    dx_s = _ext().ln_linear_bwd(g, w, x, mean, rstd, lw, lb, dres, True, *views, slab=True)
    dst = [torch.zeros(Kin, device=DEV), torch.zeros(Kin, device=DEV), torch.ones(N, Kin, device=DEV),
           torch.ones(N, device=DEV)]
    _ext().slab_reduce(slab, dst, offs)
    close(dx_s, res[1][0], 3e-2, "dx (slab)")
    for i, n in enumerate(("dgamma", "dbeta", "dW", "dbias")):
        close(dst[i], res[1][i + 1], 3e-2 if i < 3 else 1e-4, n + " (slab)")
    dst2 = [torch.zeros(Kin, device=DEV), torch.zeros(Kin, device=DEV), torch.ones(N, Kin, device=DEV),
            torch.ones(N, device=DEV)]
    dx_j = _ext().ln_linear_bwd(g, w, x, mean, rstd, lw, lb, dres, True, torch.zeros(Kin, device=DEV),
                                torch.zeros(Kin, device=DEV), None, None, job_slab=slab,
                                job_dsts=[t.view(-1) for t in dst2], job_offs=offs)
    close(dx_j, res[1][0], 3e-2, "dx (with job)")
    for i, n in enumerate(("dgamma", "dbeta", "dW", "dbias")):
        close(dst2[i], res[1][i + 1], 3e-2 if i < 3 else 1e-4, n + " (slab job)")
    # no-dx / no-LN variants
    for K in (_ext(), _emu()):
        assert K.ln_linear_bwd(g, w, x, None, None, None, None, None, False, None, None, None, None) is None
    d1 = _ext().ln_linear_bwd(g, w, x, None, None, None, None, None, True, None, None, None, None)
    d2 = _emu().ln_linear_bwd(g, w, x, None, None, None, None, None, True, None, None, None, None)
    close(d1, d2, 3e-2, "dx no-LN")
    u = bf(torch.randn(R, Kin, device=DEV))
    for mode, A in ((0, x), (1, x), (2, u)):
        outs = []
        for K in (_ext(), _emu()):
            dW, db = torch.ones(N, Kin, device=DEV), torch.ones(N, device=DEV)
            K.wgrad(g, A, mode, mean, rstd, lw, lb, 64, dW, db)
            outs.append((dW, db))
        close(outs[0][0], outs[1][0], 3e-2, f"dW mode {mode}")
        close(outs[0][1], outs[1][1], 1e-4, f"db mode {mode}")


@pytest.mark.parametrize("B,L,cap,gcap,p", [(6, 300, 96, 400, 0.15), (3, 40, 8, 12, 0.4), (64, 512, 160, 5632, 0.15)])
def test_mlm_select(B, L, cap, gcap, p):
    torch.manual_seed(8)
    lab = torch.randint(3, 1000, (B, L), device=DEV)
    lab[torch.rand(B, L, device=DEV) > p] = -100
    a = _ext().mlm_select(lab, cap, gcap)
    b = _emu().mlm_select(lab, cap, gcap)
    for x, y, n in zip(a, b, ("idx_b", "lab_b", "gidx", "glab", "total", "overflow")):
        assert torch.equal(x.cpu(), y.cpu()), n
    # with the output-query gather folded in: q = queries[idx_b] (exact copy), same selection
    queries = torch.randn(L + 3, 64, device=DEV)
    aq = _ext().mlm_select(lab, cap, gcap, None, queries)
    bq = _emu().mlm_select(lab, cap, gcap, None, queries)
    for x, y, n in zip(aq, bq, ("idx_b", "lab_b", "gidx", "glab", "total", "overflow", "q")):
        assert torch.equal(x.cpu(), y.cpu()), n + " (with queries)"


def test_stage_step_copies_and_hyper():
    """One launch copies every (dst, src) pair — 16-byte and odd sizes / offsets — and writes the
    hyper-parameter values given as kernel arguments."""
    torch.manual_seed(9)
    base = torch.randint(0, 1 << 30, (1001,), device=DEV)
    srcs = [torch.randint(0, 9000, (64, 512), device=DEV), torch.rand(64, 512, device=DEV) > 0.5,
            torch.randn(33, device=DEV), base[3:700], torch.rand(7, device=DEV) > 0.3]
    dsts = [torch.empty_like(t) for t in srcs]
    hyper = torch.full((8,), -1.0, device=DEV)
    vals = [3e-3, 17.0, 0.0, 0.9, 0.999, 0.0, 0.0, 0.0]
    _ext().stage_step(dsts, srcs, hyper, vals)
    for d, t in zip(dsts, srcs):
        assert torch.equal(d, t)
    assert torch.equal(hyper.cpu(), torch.tensor(vals, dtype=torch.float32))
    _ext().stage_step([], [], hyper, [1.0, 2.0])  # hyper only
    assert hyper[:2].tolist() == [1.0, 2.0] and hyper[2].item() == 0.0


def test_side_zero_spans():
    """ce_fwd and post_attn_bwd clear the NEXT kernel's accumulator on the way (zero_out);
    attn_bwd with dq_zeroed then matches its own-fill path."""
    torch.manual_seed(10)
    M, V, C = 300, 1000, 64
    h = torch.randn(M, C, device=DEV)
    w = bf(torch.randn(V, C, device=DEV) * 0.05)
    bias = torch.randn(V, device=DEV) * 0.01
    lab = torch.randint(0, V, (M,), device=DEV)
    cnt = torch.tensor([float(M)], device=DEV)
    z = torch.full((4 * M + 12, C), float("nan"), device=DEV)
    ref = _ext().ce_fwd(h, None, lab, w, bias, cnt)
    out = _ext().ce_fwd(h, None, lab, w, bias, cnt, z)
    assert torch.equal(z, torch.zeros_like(z))
    for x, y in zip(out, ref):
        assert torch.equal(x, y)
    # post_attn_bwd clears the cross-attention dQ buffer; attn_bwd adds into it without a fill
    B, Nq, Nk, H, D = 4, 64, 600, 4, 16
    R = B * Nq
    E = H * D
    q, k, v, km = _attn_inputs(B, B, Nq, Nk, H, D)
    scale = 1.0 / math.sqrt(D)
    o1, l1 = _ext().attn_fwd(q, k, v, km, H, D, scale, 0.0, None, 1)
    do = bf(torch.randn(B, Nq, E, device=DEV))
    g_ref = _ext().attn_bwd(q, k, v, km, o1, do, l1, None, H, D, scale, 0.0, None, None, None, None)
    ws = [bf(torch.randn(E, E, device=DEV) / 8) for _ in range(3)]
    y = torch.randn(R, E, device=DEV)
    m, r = torch.randn(R, device=DEV), torch.rand(R, device=DEV) + 0.5
    u = bf(torch.randn(R, E, device=DEV))
    g2, be2 = torch.randn(E, device=DEV), torch.randn(E, device=DEV)
    dz = torch.randn(R, E, device=DEV)
    names = ("dWo", "dbo", "dg2", "dbe2", "dW1", "db1", "dW2", "db2")
    outs = []
    dq = torch.full((B, Nq, E), float("nan"), device=DEV)
    for zo in (None, dq):
        grads = [torch.zeros((E, E) if n.startswith("dW") else (E,), device=DEV) for n in names]
        outs.append(_ext().post_attn_bwd(dz, y, m, r, u, o1.view(R, E), ws[0], ws[1], ws[2], g2, be2, H, grads,
                                         zero_out=zo))
    assert torch.equal(dq, torch.zeros_like(dq))
    for a_, b_ in zip(*outs):
        assert torch.equal(a_, b_)
    g_pre = _ext().attn_bwd(q, k, v, km, o1, do, l1, None, H, D, scale, 0.0, None, dq, None, None, dq_zeroed=True)
    for a_, b_, n in zip(g_pre, g_ref, ("dq", "dk", "dv")):
        close(a_, b_, 1e-5, n + " (pre-zeroed dq)")


@pytest.mark.parametrize("R,M,npix,kin,tall", [(6 * 100, 100, 3, 133, False), (2 * 70000, 70000, 1, 131, True)])
def test_split_pe_input_projection(R, M, npix, kin, tall):
    """Fourier-PE split input (pixels + padded PE table) for the LN+projection forward, its
    backward (incl. the tall-R weight-gradient path) and the standalone weight gradient."""
    torch.manual_seed(9)
    N = 64 if tall else 256
    pe = torch.zeros(M, (kin + 7) // 8 * 8, device=DEV)
    pe[:, npix:kin] = torch.randn(M, kin - npix, device=DEV)
    pix = torch.randn(R, npix, device=DEV)
    wp = torch.zeros(N, (kin + 7) // 8 * 8, device=DEV)
    wp[:, :kin] = torch.randn(N, kin, device=DEV) / math.sqrt(kin)
    w = bf(wp)
    lw, lb, bias = torch.randn(kin, device=DEV), torch.randn(kin, device=DEV), torch.randn(N, device=DEV)
    outs = [K.ln_linear_fwd(pix, lw, lb, 1e-5, w, bias, 0, None, True, True, pe, kin) for K in (_ext(), _emu())]
    for a, b, n in zip(outs[0], outs[1], ("y", "mean", "rstd")):
        close(a, b, 2e-2 if n == "y" else 1e-3, n)
    y, mean, rstd = outs[1]
    g = torch.randn(R, N, device=DEV)
    res = []
    for K in (_ext(), _emu()):
        dg, dbn = torch.zeros(kin, device=DEV), torch.zeros(kin, device=DEV)
        dW, dbias = torch.zeros(N, kin, device=DEV), torch.zeros(N, device=DEV)
        K.ln_linear_bwd(g, w, pix, mean, rstd, lw, lb, None, False, dg, dbn, dW, dbias, pe, kin)
        dW2, db2 = torch.ones(N, kin, device=DEV), torch.ones(N, device=DEV)
        K.wgrad(g, pix, 1, mean, rstd, lw, lb, 0, dW2, db2, pe, kin)
        res.append((dg, dbn, dW, dbias, dW2, db2))
    for a, b, n in zip(res[0], res[1], ("dgamma", "dbeta", "dW", "dbias", "wgrad dW", "wgrad db")):
        close(a, b, 3e-2, n)


def test_split_pe_input_gathered_rows():
    """The split input with a row index (pe_index: row r reads pe[pe_index[r]], the sparse images'
    gathered rows) through the forward, the backward and the standalone weight gradient, at an odd
    input width (131) over two 64-row tiles."""
    torch.manual_seed(19)
    R, M, npix, kin, N = 128, 50, 1, 131, 64
    pe = torch.zeros(M, (kin + 7) // 8 * 8, device=DEV)
    pe[:, npix:kin] = torch.randn(M, kin - npix, device=DEV)
    idx = torch.randint(0, M, (R,), device=DEV)
    pix = torch.randn(R, npix, device=DEV)
    wp = torch.zeros(N, (kin + 7) // 8 * 8, device=DEV)
    wp[:, :kin] = torch.randn(N, kin, device=DEV) / math.sqrt(kin)
    w = bf(wp)
    lw, lb, bias = torch.randn(kin, device=DEV), torch.randn(kin, device=DEV), torch.randn(N, device=DEV)
    outs = [K.ln_linear_fwd(pix, lw, lb, 1e-5, w, bias, 0, None, True, True, pe, kin, idx) for K in (_ext(), _emu())]
    for a, b, n in zip(outs[0], outs[1], ("y", "mean", "rstd")):
        close(a, b, 2e-2 if n == "y" else 1e-3, n)
    y, mean, rstd = outs[1]
    g = torch.randn(R, N, device=DEV)
    res = []
    for K in (_ext(), _emu()):
        dg, dbn = torch.zeros(kin, device=DEV), torch.zeros(kin, device=DEV)
        dW, dbias = torch.zeros(N, kin, device=DEV), torch.zeros(N, device=DEV)
        K.ln_linear_bwd(g, w, pix, mean, rstd, lw, lb, None, False, dg, dbn, dW, dbias, pe, kin, pe_index=idx)
        dW2, db2 = torch.ones(N, kin, device=DEV), torch.ones(N, device=DEV)
        K.wgrad(g, pix, 1, mean, rstd, lw, lb, 0, dW2, db2, pe, kin, idx)
        res.append((dg, dbn, dW, dbias, dW2, db2))
    for a, b, n in zip(res[0], res[1], ("dgamma", "dbeta", "dW", "dbias", "wgrad dW", "wgrad db")):
        close(a, b, 3e-2, n)


def test_ln_linear_bwd_dx_in_place_of_dres():
    """dx_out naming the dres buffer itself: dX = LN_bwd(g·w) + dres lands in place (the latent
    array's gradient in the cross-attention backward)."""
    torch.manual_seed(20)
    R, N, Kin = 128, 64, 64
    g = torch.randn(R, N, device=DEV)
    w = bf(torch.randn(N, Kin, device=DEV) / math.sqrt(Kin))
    x = torch.randn(R, Kin, device=DEV) * 1.5 + 0.2
    lw, lb = torch.randn(Kin, device=DEV), torch.randn(Kin, device=DEV)
    mean, rstd = x.mean(-1), torch.rsqrt(x.var(-1, unbiased=False) + 1e-5)
    dres = torch.randn(R, Kin, device=DEV)
    res = []
    for K in (_ext(), _emu()):
        buf = dres.clone()
        dg, db = torch.zeros(Kin, device=DEV), torch.zeros(Kin, device=DEV)
        dx = K.ln_linear_bwd(g, w, x, mean, rstd, lw, lb, buf, True, dg, db, None, None, dx_out=buf)
        assert dx.data_ptr() == buf.data_ptr()
        res.append((buf, dg, db))
    for a, b, n in zip(res[0], res[1], ("dx", "dgamma", "dbeta")):
        close(a, b, 3e-2, n)


# (1552, 2003) and (900, 3000): split counts that used to leave trailing vocab splits without
# a chunk (an empty split read its rows' dH targets from LDS before any barrier)
# (300, 256), (1000, 2) and (33, 3) at C = 64: a vocabulary of at most 256 entries (the two-pass
# backward's one-hot-in-tile instance) with two, one and one partial vocabulary block, and 5, 32
# and 2 appended dH grid rows
@pytest.mark.parametrize("M,V,C", [(300, 1000, 64), (77, 10003, 64), (64, 257, 128), (1552, 2003, 64),
                                   (900, 3000, 32), (300, 256, 64), (1000, 2, 64), (33, 3, 64)])
def test_fused_cross_entropy(M, V, C):
    torch.manual_seed(5)
    h = bf(torch.randn(M, C, device=DEV))
    w = bf(torch.randn(V, C, device=DEV) * 0.3)
    bias = torch.randn(V, device=DEV) * 0.1
    lab = torch.randint(0, V, (M,), device=DEV)
    lab[::7] = -100
    hf = h.float()  # bf16-exact fp32 rows (the kernels cast on load)
    cnt = torch.tensor([float((lab >= 0).sum())], device=DEV)
    l2, s2, hs2 = _emu().ce_fwd(hf, None, lab, w, bias, cnt)[:3]
    u = {}  # C = 64: the two-pass head's per-split Σ p·W partials and (max, sum) pairs feed ce_bwd
    for _ in range(3):  # the row-block and loss tickets are re-armed by every launch
        o = _ext().ce_fwd(hf, None, lab, w, bias, cnt)
        l1, s1, hs1 = o[:3]
        u = dict(u=o[3], u_ml=o[4]) if len(o) > 4 else {}
        assert rel_fro(l1, l2) < 1e-3 and rel_fro(s1, s2) < 1e-3, (rel_fro(l1, l2), rel_fro(s1, s2))
        assert torch.equal(hs1, hs2)
    assert bool(u) == (C == 64)
    # gathered rows: row r of the head input is hbig[idx[r]]
    idx = torch.randperm(2 * M, device=DEV)[:M]
    hbig = torch.zeros(2 * M, C, device=DEV)
    hbig[idx] = hf
    o = _ext().ce_fwd(hbig, idx, lab, w, bias, cnt)
    lg, sg, hsg = o[:3]
    assert rel_fro(lg, l2) < 1e-3 and rel_fro(sg, s2) < 1e-3
    assert torch.equal(hsg, hs2)  # the compact rows: gathered and cast on load
    # count_labels: the head counts the labelled rows itself (classifier heads)
    cnt_out = torch.full((1,), -5.0, device=DEV)
    lc = _ext().ce_fwd(hf, None, lab, w, bias, cnt_out, None, True)[0]
    assert cnt_out.item() == cnt.item() and rel_fro(lc, l2) < 1e-3
    gout = torch.tensor([0.37], device=DEV)
    rowmap = torch.randperm(3 * M, device=DEV)[:M]  # scatter rows into a larger (3M, C) gradient
    outs = []
    for K in (_ext(), _emu()):
        dH = torch.zeros(M, C, device=DEV)
        dW = torch.full((V, C), 7.0, device=DEV)  # overwritten (accumulate=False)
        db = torch.zeros(V, device=DEV)
        K.ce_bwd(hs2, lab, w, bias, s2, gout, cnt, dH, dW, db, False, None, **u)
        dHs = torch.zeros(3 * M, C, device=DEV)
        dW2, db2 = dW.clone(), db.clone()
        K.ce_bwd(hs2, lab, w, bias, s2, gout, cnt, dHs, dW2, db2, True, rowmap, **u)
        sl = K.ce_bwd(hs2, lab, w, bias, s2, gout, cnt, torch.zeros(M, C, device=DEV), dW.clone(), db.clone(), False,
                      None, slab=True, **u)
        slab_sum = sl.sum(0)
        outs.append((dH, dW, db, dHs, dW2, db2, slab_sum[:V * C].view(V, C), slab_sum[V * C:V * C + V]))
    names = ("dH", "dW", "db", "dH rowmap", "dW acc", "db acc", "dW slab", "db slab")
    errs = {n: rel_fro(a, b) for a, b, n in zip(outs[0], outs[1], names)}
    assert all(e < 1e-2 for e in errs.values()), errs
    if C == 64:  # the two-pass head has no backward without the forward's split partials
        with pytest.raises(RuntimeError, match="needs u and u_ml"):
            _ext().ce_bwd(hs2, lab, w, bias, s2, gout, cnt, torch.zeros(M, C, device=DEV), dW, db, False, None)


def test_embed_mask_adamw():
    torch.manual_seed(6)
    B, L, V, C = 4, 50, 300, 64
    ids = torch.randint(0, V, (B, L), device=DEV)
    ids[:, ::3] = 2  # a very frequent id (like [MASK]): long equal-id runs after sorting
    E, P = torch.randn(V, C, device=DEV), torch.randn(64, C, device=DEV)
    close(_ext().embed_fwd(ids, E, P[:L].contiguous(), 8.0), _emu().embed_fwd(ids, E, P[:L].contiguous(), 8.0), 1e-6, "emb")
    # embedding backward: small ragged batch, and multi-block batches (block-local sort + run
    # folding across 256-token blocks, partial last block), C = 64 and 128
    for (Bb, Lb, Cb) in ((B, L, C), (8, 512, 64), (3, 333, 128)):
        idb = torch.randint(0, V, (Bb, Lb), device=DEV)
        idb[:, ::3] = 2
        idb[:, 1::7] = 0
        g = torch.randn(Bb, Lb, Cb, device=DEV)
        r = []
        for K in (_ext(), _emu()):
            dE, dP = torch.ones(V, Cb, device=DEV), torch.zeros(Lb, Cb, device=DEV)
            K.embed_bwd(idb, g, dE, dP, 8.0)
            r.append((dE, dP))
        close(r[0][0], r[1][0], 1e-5, f"dE {Bb}x{Lb}x{Cb}")
        close(r[0][1], r[1][1], 1e-5, f"dP {Bb}x{Lb}x{Cb}")
    x = torch.randint(0, V, (B, L), device=DEV)
    pad = torch.rand(B, L, device=DEV) < 0.2
    # counter-hash masking: bit-exact with the emulation, and the kernel advances the counter
    # (ticket reset) so consecutive launches draw different masks
    st_k = torch.tensor([0x123456789AB, 5, 0], device=DEV)
    st_e = st_k.clone()
    for _ in range(3):
        a = _ext().text_mask(x, pad, st_k, 1, 2, 0.15, 3, V, True)
        b = _emu().text_mask(x, pad, st_e, 1, 2, 0.15, 3, V, True)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert torch.equal(st_k, st_e) and int(st_k[2]) == 0
    assert int(st_k[1]) == 8
    c = _ext().text_mask(x, pad, st_k, 1, 2, 0.15, 3, V, False)
    assert not torch.equal(c[1], a[1]) and int(st_k[1]) == 8
    n = 10000
    res = []
    for K in (_ext(), _emu()):
        torch.manual_seed(7)
        p, gg = torch.randn(n, device=DEV), torch.randn(n, device=DEV)
        m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        sh = torch.zeros(n, device=DEV, dtype=torch.bfloat16)
        hyper = torch.tensor([1e-3, 1.0, 0.0, 0.9, 0.999, 0, 0, 0], device=DEV)
        part = torch.full((512,), float("nan"), device=DEV)
        K.sumsq(gg, part)
        K.adamw(p, gg, m, v, sh, hyper, 1e-8, 0.01, 1.0, 1.0, norm_part=part)
        res.append((p, m, v, sh))
    for a_, b_, nme in zip(res[0], res[1], ("p", "m", "v", "shadow")):
        close(a_, b_, 1e-5, nme)


@pytest.mark.parametrize("channels,B,M,O", [(3, 2, 50176, 256), (1, 4, 784, 256), (4, 3, 1000, 512), (2, 5, 333, 128),
                                              (2, 130, 40, 128)])
def test_factored_pe_projection_kernels(channels, B, M, O):
    """csrc/pe_proj.hip forward epilogue + streaming backward vs fp64 autograd of LayerNorm +
    Linear over the materialised [pixels ‖ PE] rows (ImageNet shape first: M = 224·224)."""
    from test_models import check_factored_pe_projection

    check_factored_pe_projection(_ext(), "cuda", channels, B=B, M=M, O=O)


@pytest.mark.parametrize("B,Bq,Nq,M,H,nc,bsplit", [
    (3, 1, 32, 600, 4, 3, 1),
    (4, 1, 17, 300, 4, 1, 2),
    (2, 1, 32, 50176, 4, 3, 1),
    (8, 1, 32, 784, 2, 4, 8),
    (3, 3, 32, 600, 4, 3, 1),
    (2, 2, 32, 50176, 4, 3, 1),
    (8, 8, 20, 784, 4, 1, 4),
])
def test_attention_bwd_pe_fused(B, Bq, Nq, M, H, nc, bsplit):
    """Cross-attention backward folded into the factored projection's reductions
    (attention_pe.hip) vs the emulation (attn_bwd → pe_proj_bwd), incl. a second accumulating
    application (weight-shared layer_n) and batch groups (atomics on D)."""
    torch.manual_seed(9)
    C = 32 * H
    q = bf(torch.randn(Bq, Nq, 3 * C, device=DEV))[:, :, :C]
    kv = bf(torch.randn(B * M, 2 * C, device=DEV))
    dO = bf(torch.randn(B, Nq, C, device=DEV))
    scale = 1 / math.sqrt(32)
    kv3 = kv.view(B, M, 2 * C)
    o, lse = _emu().attn_fwd(q, kv3[:, :, :C], kv3[:, :, C:], None, H, 32, scale, 0.0, None, 1)
    delta = (dO.float().view(B, Nq, H, 32) * o.float().view(B, Nq, H, 32)).sum(-1).contiguous()
    pix = torch.randn(B * M, nc, device=DEV)
    mean = torch.randn(B * M, device=DEV) * 0.1
    rstd = torch.rand(B * M, device=DEV) + 0.5
    nkb = (M + 255) // 256
    res = []
    for K in (_ext(), _emu()):
        dq = torch.empty(Bq, Nq, C, device=DEV)
        D = torch.empty(M, 2 * C, device=DEV)
        part = torch.empty(K.attn_bwd_pe_part_rows(M, H, B, bsplit), (2 + nc) * 2 * C, device=DEV)
        K.attn_bwd_pe(q, kv, dO, lse, delta, mean, rstd, pix, dq, D, part, H, scale, False, bsplit)
        dq1 = dq.clone()
        K.attn_bwd_pe(q, kv, dO, lse, delta, mean, rstd, pix, dq, D, part, H, scale, True, bsplit)
        res.append((dq1, dq, D, part.sum(0)))
    for a, b, n in zip(res[0], res[1], ("dq", "dq (2nd)", "D (2 applications)", "partials")):
        close(a, b, 2e-2, n)


def _pe_implicit_operands(M, H, nc, kin=133):
    """Realistic operands of the implicit K/V: a Fourier-like PE table (Σe, Σe² → LayerNorm
    statistics with the pixels), W ~ N(0, 1/kin) so K/V are O(1), and P' = Ebf·(W⊙γ)ᵀ in bf16."""
    C = 32 * H
    E = torch.rand(M, kin - nc, device=DEV) * 2 - 1
    W = torch.randn(2 * C, kin, device=DEV) / math.sqrt(kin)
    g, b = 1 + 0.1 * torch.randn(kin, device=DEV), 0.1 * torch.randn(kin, device=DEV)
    bias = 0.1 * torch.randn(2 * C, device=DEV)
    Kp = -(-kin // 32) * 32
    Ebf = torch.zeros(M, Kp, device=DEV)
    Ebf[:, nc:kin] = E
    Ebf = bf(Ebf)
    wg, _, _, _, wt = _emu().pe_weight_prep(W, g, b, bias, nc, Kp)
    if (2 * C) % 128 == 0:  # 64 zero pad rows: the forward's last prefetch reads past M
        P = _ext().pe_gemm(Ebf, wg, bf16_out=True, pad_rows=64)
        assert torch.equal(P[M:].float(), torch.zeros(64, 2 * C, device=DEV))
    else:
        P = _emu().pe_gemm(Ebf, wg, bf16_out=True, pad_rows=64)
    return P, E.sum(1).contiguous(), (E * E).sum(1).contiguous(), wt, kin


def _pe_fwd_fp32(q, P, pix, pes, pesq, wt, H, scale, kin, eps):
    """fp32 reference of the implicit-K/V cross-attention: K/V rows (pe_kv_elem) in fp32 from the
    bf16 P', softmax attention in fp32 → O (B, Nq, C), LSE (B, Nq, H) in log2 units."""
    C, M = H * 32, pes.shape[0]
    B, nc = pix.shape[0] // M, pix.shape[1]
    m = torch.arange(B * M, device=pix.device) % M
    mu = (pes[m] + pix.sum(1)) / kin
    rs = torch.rsqrt(((pesq[m] + (pix * pix).sum(1)) / kin - mu * mu).clamp(min=0) + eps)
    y = rs[:, None] * (P[m].float() + (pix - mu[:, None]) @ wt[:nc] + mu[:, None] * wt[4]) + wt[5]
    kv = y.view(B, M, 2, H, 32)
    qf = q.float().expand(B, -1, -1).reshape(B, -1, H, 32)
    s = torch.einsum("bqhd,bmhd->bhqm", qf, kv[:, :, 0]) * scale
    o = torch.einsum("bhqm,bmhd->bqhd", torch.softmax(s, -1), kv[:, :, 1]).reshape(B, -1, C)
    return o, (torch.logsumexp(s, -1) / math.log(2)).permute(0, 2, 1).contiguous()


@pytest.mark.parametrize("B,Bq,Nq,M,H,nc,bsplit,nsplit", [
    (3, 1, 32, 600, 4, 3, 1, 7),
    (4, 1, 17, 300, 4, 1, 2, 3),
    (2, 1, 32, 50176, 4, 3, 1, 64),
    (8, 1, 32, 784, 2, 4, 8, 5),
    (3, 3, 32, 600, 4, 3, 1, 1),
    (2, 2, 32, 50176, 4, 3, 1, 32),
    (5, 5, 20, 784, 4, 1, 4, 25),
    (2, 1, 32, 288, 4, 3, 1, 4),   # the last split is empty
    (6, 6, 32, 1000, 4, 2, 1, 0),  # 0: the kernel's own split count
])
def test_attention_pe_implicit_kv(B, Bq, Nq, M, H, nc, bsplit, nsplit):
    """Encoder cross-attention over implicit K/V (attention_pe.hip attn_fwd_pe_kernel and the IMPL
    backward: K/V tiles generated from P', pixels and the table, never materialised) vs the
    emulation (materialised pe_kv → attn_fwd / attn_bwd → pe_proj_bwd): O, LSE, and dq, D and
    the partials over two accumulating applications (the weight-shared layer_n)."""
    torch.manual_seed(13)
    C = 32 * H
    P, pes, pesq, wt, kin = _pe_implicit_operands(M, H, nc)
    pix = torch.randn(B * M, nc, device=DEV)
    q = bf(torch.randn(Bq, Nq, 3 * C, device=DEV))[:, :, :C]
    dO = bf(torch.randn(B, Nq, C, device=DEV))
    scale = 1 / math.sqrt(32)
    eps = 1e-5
    o1, l1 = _ext().attn_fwd_pe(q, P, pix, pes, pesq, wt, H, scale, kin, eps, nsplit)
    o2, l2 = _emu().attn_fwd_pe(q, P, pix, pes, pesq, wt, H, scale, kin, eps, 1)
    close(o1, o2, 1e-2, "O")
    # the factored forward (default) never forms the bf16 K/V the emulation rounds: judge both
    # against the fp32 reference (K/V in fp32 from the same bf16 P'), the kernel's LSE error at
    # most that of the emulation's (bf16 K/V) path plus 1e-4 of the LSE scale
    o3, l3 = _pe_fwd_fp32(q, P, pix, pes, pesq, wt, H, scale, kin, eps)
    e_kernel = (l1.float() - l3).abs().max().item()
    e_emu = (l2.float() - l3).abs().max().item()
    assert e_kernel <= 1.25 * e_emu + 1e-4 * l3.abs().max().item(), ("LSE", e_kernel, e_emu)
    close(o1, o3, 1e-2, "O vs fp32")
    delta = (dO.float().view(B, Nq, H, 32) * o2.float().view(B, Nq, H, 32)).sum(-1).contiguous()
    nkb = (M + 255) // 256
    res = []
    for K in (_ext(), _emu()):
        dq = torch.empty(Bq, Nq, C, device=DEV)
        D = torch.empty(M, 2 * C, device=DEV)
        part = torch.empty(K.attn_bwd_pe_part_rows(M, H, B, bsplit), (2 + nc) * 2 * C, device=DEV)
        K.attn_bwd_pe_implicit(q, P, pes, pesq, wt, dO, l2, delta, pix, dq, D, part, H, scale, kin, eps, False, bsplit)
        dq1 = dq.clone()
        K.attn_bwd_pe_implicit(q, P, pes, pesq, wt, dO, l2, delta, pix, dq, D, part, H, scale, kin, eps, True, bsplit)
        res.append((dq1, dq, D, part.sum(0)))
    for a, b, n in zip(res[0], res[1], ("dq", "dq (2nd)", "D (2 applications)", "partials")):
        close(a, b, 2e-2, n)


@pytest.mark.parametrize("qscale,nsplit", [(6.0, 1), (6.0, 4), (0.05, 1), (0.05, 0)])
def test_attention_pe_folded_offset_extreme_scores(qscale, nsplit):
    """The factored forward subtracts its lazy softmax offset inside the score MFMA (bf16 hi / lo
    splits of 1 / (rσ·scale_log2) against −m), not per score.  Peaked scores (queries × 6: tens
    of log2 units, the offset moving on many of the 94 chunks of a split) and near-flat ones
    (× 0.05) — O and the LSE against the fp32 reference."""
    torch.manual_seed(17)
    H, nc, M, B, Nq = 4, 3, 3000, 3, 32
    C = 32 * H
    P, pes, pesq, wt, kin = _pe_implicit_operands(M, H, nc)
    pix = torch.randn(B * M, nc, device=DEV)
    q = bf(torch.randn(B, Nq, C, device=DEV) * qscale)
    scale = 1 / math.sqrt(32)
    o1, l1 = _ext().attn_fwd_pe(q, P, pix, pes, pesq, wt, H, scale, kin, 1e-5, nsplit)
    o3, l3 = _pe_fwd_fp32(q, P, pix, pes, pesq, wt, H, scale, kin, 1e-5)
    close(o1, o3, 2e-2, "O vs fp32")
    err, top = (l1.float() - l3).abs().max().item(), l3.abs().max().item()
    assert err <= 1e-3 * top + 5e-3, ("LSE", err, top)


def test_index_add_rows_and_sumsq():
    torch.manual_seed(11)
    dst = torch.randn(1000, 64, device=DEV)
    idx = torch.randint(0, 1000, (5000,), device=DEV)  # repeated rows
    src = torch.randn(5000, 64, device=DEV)
    ref = dst.clone().index_add_(0, idx, src)
    _ext().index_add_rows(dst, idx, src)
    close(dst, ref, 1e-5, "index_add_rows")
    got = _ext().gather_rows(src, idx[:3000] % 5000)  # the forward gather (bitwise a copy)
    assert torch.equal(got, src.index_select(0, idx[:3000] % 5000))
    for n in (1, 1000, 17 * 1024 * 1024 + 3):
        g = torch.randn(n, device=DEV)
        part = torch.full((512,), float("nan"), device=DEV)  # every partial is written
        _ext().sumsq(g, part)
        ref = (g.double() ** 2).sum().float()
        assert abs(part.sum().item() - ref.item()) <= 1e-4 * ref.item(), (n, part.sum().item(), ref.item())
        again = torch.empty_like(part)
        _ext().sumsq(g, again)
        assert torch.equal(part, again)  # fixed order, no atomics: bitwise reproducible
    g = torch.randn(4097, device=DEV)[1:]  # 4-byte aligned, not 16: scalar path
    part = torch.zeros(512, device=DEV)
    _ext().sumsq(g, part)
    assert abs(part.sum().item() - (g.double() ** 2).sum().item()) <= 1e-4 * part.sum().item()


@pytest.mark.parametrize("R,C,K", [(5000, 64, 3), (333, 32, 2), (1000, 128, 4), (17, 64, 3)])
def test_pixel_ce_kernels(R, C, K):
    """Fused per-pixel head + weighted CE (pixel_head.hip) vs the fp32 emulation."""
    torch.manual_seed(12)
    h = torch.randn(R, C, device=DEV)
    W = torch.randn(K, C, device=DEV) * 0.3
    b = torch.randn(K, device=DEV) * 0.1
    lab = torch.randint(0, K, (R,), device=DEV)
    lab[::5] = -100
    wts = torch.rand(K, device=DEV) + 0.5
    wts[0] = 0.0
    (t1, l1), (t2, l2) = _ext().pixel_ce_fwd(h, W, b, lab, wts), _emu().pixel_ce_fwd(h, W, b, lab, wts)
    close(t1[:2], t2[:2], 1e-4, "loss sums")
    close(l1, l2, 1e-4, "loss")
    ns = 4 + 2 * K
    assert torch.equal(t1[2:ns], t2[2:ns]), (t1[2:ns], t2[2:ns])  # counts / hits exact
    close(t1[ns:], t2[ns:], 1e-6, "accuracies")
    gout = torch.tensor([0.7], device=DEV)
    res = []
    for Kx in (_ext(), _emu()):
        d = torch.empty_like(h)
        dW, db = torch.ones(K, C, device=DEV), torch.ones(K, device=DEV)  # accumulated onto
        Kx.pixel_ce_bwd(h, W, b, lab, wts, gout, t2, d, dW, db)
        res.append((d, dW, db))
    for a, c, n in zip(res[0], res[1], ("dH", "dW", "db")):
        close(a, c, 1e-4, n)


@pytest.mark.parametrize("M,N,K", [(50176, 256, 288), (1000, 128, 32), (333, 384, 96)])
def test_pe_gemm_and_weight_prep(M, N, K):
    """In-tree PE GEMM (bf16 operands, fp32 accumulate / output) and the per-step weight prep of
    the factored K/V projection, against fp32 torch references."""
    torch.manual_seed(9)
    A = bf(torch.rand(M, K, device=DEV) * 2 - 1)
    A[:, :3] = 0
    B = bf(torch.randn(N, K, device=DEV) * 0.1)
    c1 = _ext().pe_gemm(A, B)
    c2 = A.float() @ B.float().t()
    close(c1, c2, 1e-4, "pe_gemm")
    c3 = _ext().pe_gemm(A, B, bf16_out=True)  # the implicit-K/V operand P'
    assert c3.dtype == torch.bfloat16 and torch.equal(c3, c1.to(torch.bfloat16))
    kin, nc = K - 5, 3
    W = torch.randn(N, kin, device=DEV)
    g, b = torch.randn(kin, device=DEV), torch.randn(kin, device=DEV)
    bias = torch.randn(N, device=DEV)
    r1 = _ext().pe_weight_prep(W, g, b, bias, nc, K)
    r2 = _emu().pe_weight_prep(W, g, b, bias, nc, K)
    for x, y, n in zip(r1, r2, ("Wg", "wpg", "gw", "bw", "wt")):
        close(x, y, 1e-5, n)
    # separate K / V weights read in place (no concatenation): bitwise the stacked call
    r3 = _ext().pe_weight_prep(W[: N // 2].contiguous(), g, b, bias, nc, K, W[N // 2:].contiguous())
    for x, y, n in zip(r3, r1, ("Wg", "wpg", "gw", "bw", "wt")):
        assert torch.equal(x, y), n


@pytest.mark.parametrize("M,O,Kp,kin,nc,nblk", [(50176, 256, 288, 261, 3, 37), (784, 256, 160, 131, 1, 5),
                                               (1000, 64, 96, 70, 2, 3)])
def test_pe_grads(M, O, Kp, kin, nc, nblk):
    """Factored-projection weight / LN gradients (pe_gemm_tn → reduce → finalize), added into
    pre-filled targets, against the emulation."""
    torch.manual_seed(10)
    D = torch.randn(M, O, device=DEV)
    part = torch.randn(nblk, (2 + nc) * O, device=DEV)
    E = torch.zeros(M, Kp, device=DEV)
    E[:, nc:kin] = torch.rand(M, kin - nc, device=DEV) * 2 - 1
    E = bf(E)
    Ch = O // 2
    Wa, Wb = torch.randn(Ch, kin, device=DEV), torch.randn(O - Ch, kin, device=DEV)
    g, b = torch.randn(kin, device=DEV), torch.randn(kin, device=DEV)
    outs = []
    for K in (_ext(), _emu()):
        t = [torch.full((Ch, kin), 0.5, device=DEV), torch.full((O - Ch, kin), 0.5, device=DEV),
             torch.ones(O, device=DEV), torch.ones(kin, device=DEV), torch.ones(kin, device=DEV)]
        K.pe_grads(D, part, E, Wa, Wb, g, b, nc, *t)
        outs.append(t)
    for a, c, n in zip(outs[0], outs[1], ("dWa", "dWb", "db", "dgamma", "dbeta")):
        close(a, c, 2e-3, n)


@pytest.mark.parametrize("B,N,nxt", [(4, 256, True), (3, 128, False), (2, 64, True)])
def test_sa_layer_fwd_fused(B, N, nxt):
    """Fused self-attention layer forward (attention + post-attention block + next LN1/QKV in one
    launch) against the emulation's composition of the separate ops."""
    torch.manual_seed(12)
    C, R = 64, B * N
    qkv = bf(torch.randn(R, 3 * C, device=DEV))
    x = torch.randn(R, C, device=DEV)

    def w(*s, sc=0.15):
        return bf(torch.randn(*s, device=DEV) * sc)

    wo, w1, w2 = w(C, C), w(C, C), w(C, C)
    bo, b1, b2 = (torch.randn(C, device=DEV) * 0.1 for _ in range(3))
    g2, be2 = 1 + 0.1 * torch.randn(C, device=DEV), 0.1 * torch.randn(C, device=DEV)
    extra = {}
    if nxt:
        extra = dict(lnw=1 + 0.1 * torch.randn(C, device=DEV), lnb=0.1 * torch.randn(C, device=DEV), wq=w(3 * C, C),
                     bq=0.1 * torch.randn(3 * C, device=DEV))
    a = _ext().sa_layer_fwd(qkv, x, N, 0.25, wo, bo, g2, be2, 1e-5, w1, b1, w2, b2, **extra)
    e = _emu().sa_layer_fwd(qkv, x, N, 0.25, wo, bo, g2, be2, 1e-5, w1, b1, w2, b2, **extra)
    names = ["o", "lse", "z", "y", "mean2", "rstd2", "u"] + (["qkv_next", "mean1", "rstd1"] if nxt else [])
    assert len(a) == len(e) == len(names)
    for u, v, n in zip(a, e, names):
        # the next layer's LN1 statistics come from z, after the bf16 GEMM chain: 1 %
        close(u, v, 1e-3 if n in ("lse", "mean2", "rstd2") else 1e-2 if n in ("mean1", "rstd1") else 2e-2, n)


_CHECKED_PROBE = r"""
import torch
from perceiver_io_amd.ops import ext
K = ext.require()
assert K.checked_build() and K.__name__.endswith("_C_check"), K.__name__
dev = "cuda"
E, P = torch.randn(50, 64, device=dev), torch.randn(8, 64, device=dev)
ok = K.embed_fwd(torch.randint(0, 50, (2, 8), device=dev), E, P, 1.0)
assert K.check_errors(True) == 0
out = []
for name, fn in (
        ("embed", lambda: K.embed_fwd(torch.tensor([[3, 50, 1, 2, 0, 0, 0, 0]], device=dev), E, P, 1.0)),
        ("label", lambda: K.ce_fwd(torch.randn(4, 64, device=dev), None, torch.tensor([1, 2, 1000, -100], device=dev),
                                   torch.randn(100, 64, device=dev).to(torch.bfloat16), torch.zeros(100, device=dev),
                                   torch.tensor([3.0], device=dev))),
        ("gather", lambda: K.index_add_rows(torch.zeros(10, 64, device=dev), torch.tensor([1, 12], device=dev),
                                            torch.ones(2, 64, device=dev))),
        # a sparse image's PE row index past the table (rowgemm.hip pe_row)
        ("pe_index", lambda: K.ln_linear_fwd(torch.randn(64, 1, device=dev), torch.ones(32, device=dev),
                                             torch.zeros(32, device=dev), 1e-5,
                                             torch.randn(64, 32, device=dev).to(torch.bfloat16), None, 0, None, True,
                                             True, torch.randn(100, 32, device=dev), 32,
                                             torch.tensor([3] * 63 + [100], device=dev)))):
    try:
        fn()
        out.append((name, "no error"))
    except RuntimeError as e:
        out.append((name, "checked build" in str(e)))
torch.cuda.synchronize()
# inside a replayed hipGraph no launch can raise: the sticky words are read by
# ops.check_device_errors() (the Trainer's logging-step / end-of-fit check, bench.py after timing)
from perceiver_io_amd import ops
ids = torch.randint(0, 50, (1, 8), device=dev)
K.embed_fwd(ids, E, P, 1.0)
torch.cuda.synchronize()
g = torch.cuda.CUDAGraph()
with torch.cuda.graph(g):
    K.embed_fwd(ids, E, P, 1.0)
ops.check_device_errors()  # clean after a valid capture
ids[0, 1] = 50
g.replay()
torch.cuda.synchronize()
try:
    ops.check_device_errors()
    out.append(("graph", "no error"))
except RuntimeError as e:
    out.append(("graph", "checked build" in str(e)))
print(out)
assert all(r is True for _, r in out), out
assert K.check_errors(True) == 0
print("CHECKED_OK")
"""


def test_checked_build_flags_out_of_range_indices():
    """The checked variant (build.py --check → _C_check, PERCEIVER_CHECKED=1) validates token ids,
    class labels and gather rows on the device: the access is clamped / skipped and the call
    raises; valid inputs pass.  Runs in a child process (the loaded variant is process-wide)."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PERCEIVER_CHECKED="1", PYTHONPATH=root)
    r = subprocess.run([sys.executable, "-c", _CHECKED_PROBE], env=env, capture_output=True, text=True, timeout=240,
                       cwd=root)
    assert r.returncode == 0 and "CHECKED_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


def rel_fro(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _slab_sum(sl):
    """per-segment totals of a (tiles, P) slab (what slab_reduce adds into the gradients)"""
    tot = sl.t.float().sum(0)
    return [tot[o:o + n] for o, n in zip(sl.offs, sl.sizes)]


@pytest.mark.parametrize("nq,p,R", [(192, 0.0, 512), (192, 0.1, 256), (64, 0.0, 320)])
def test_ln_linear_post_attn_bwd_isolated(nq, p, R):
    """The layer-boundary backward (LN1/QKV backward of layer l+1 fused with the post-attention
    backward of layer l; 30 % of the headline step) in isolation against the emulation: every
    output and every slab-reduced parameter gradient within 1 % relative Frobenius error."""
    from perceiver_io_amd.ops.fused import LL_SIZES, PA_SIZES, _GradSlab

    torch.manual_seed(21)
    C, H = 64, 4
    eps = 1e-5

    def w(*s, sc=0.15):
        return bf(torch.randn(*s, device=DEV) * sc)

    x = torch.randn(R, C, device=DEV)
    mean1, rstd1 = x.mean(1), torch.rsqrt(x.var(1, unbiased=False) + eps)
    y = torch.randn(R, C, device=DEV)
    m2, r2 = y.mean(1), torch.rsqrt(y.var(1, unbiased=False) + eps)
    g = torch.randn(R, nq, device=DEV)
    dres = torch.randn(R, C, device=DEV)
    u, o = bf(torch.randn(R, C, device=DEV)), bf(torch.randn(R, C, device=DEV))
    wq, wo, w1, w2 = w(nq, C), w(C, C), w(C, C), w(C, C)
    lnw, lnb = 1 + 0.1 * torch.randn(C, device=DEV), 0.1 * torch.randn(C, device=DEV)
    g2, be2 = 1 + 0.1 * torch.randn(C, device=DEV), 0.1 * torch.randn(C, device=DEV)
    seed = torch.tensor([1234567], dtype=torch.int64, device=DEV) if p > 0 else None
    res = {}
    for name, K in (("hip", _ext()), ("emu", _emu())):
        sl = _GradSlab(R, [C, C, nq * C, nq] + PA_SIZES(C), x)
        sl.t.fill_(float("nan") if name == "hip" else 0.0)
        tg = sl.targets()
        outs = K.ln_linear_post_attn_bwd(g, wq, x, mean1, rstd1, lnw, lnb, dres, tg[:4], y, m2, r2, u, o, wo, w1, w2,
                                         g2, be2, H, tg[4:], seed=seed, site=3, p=p)
        if name == "hip":
            assert torch.isfinite(sl.t).all()  # every tile stored every element of its slab row
        res[name] = list(outs) + _slab_sum(sl)
    names = ["dy", "dO", "delta", "dlnw", "dlnb", "dWq", "dbq", "dWo", "dbo", "dg2", "dbe2", "dW1", "db1", "dW2", "db2"]
    errs = {n: rel_fro(a, b) for n, a, b in zip(names, res["hip"], res["emu"])}
    bad = {n: e for n, e in errs.items() if not e < 1e-2}
    assert not bad, errs


@pytest.mark.parametrize("B,N,nq,p", [(4, 256, 64, 0.0), (2, 128, 128, 0.1), (3, 64, 192, 0.1), (2, 256, 0, 0.1),
                                     (2, 512, 192, 0.0), (3, 320, 0, 0.1)])
def test_sa_layer_fwd_widths_and_dropout(B, N, nq, p):
    """The fused self-attention layer forward for every next-projection width the encoder uses
    (a cross layer's query projection C, a decoder's K/V 2C, the next layer's QKV 3C; 0 = last
    layer) with residual dropout, per output within 1 % relative Frobenius error; N up to the
    long-context MLM's 512 latents (16 key tiles)."""
    torch.manual_seed(13)
    C, R = 64, B * N
    qkv = bf(torch.randn(R, 3 * C, device=DEV))
    x = torch.randn(R, C, device=DEV)

    def w(*s, sc=0.15):
        return bf(torch.randn(*s, device=DEV) * sc)

    wo, w1, w2 = w(C, C), w(C, C), w(C, C)
    bo, b1, b2 = (torch.randn(C, device=DEV) * 0.1 for _ in range(3))
    g2, be2 = 1 + 0.1 * torch.randn(C, device=DEV), 0.1 * torch.randn(C, device=DEV)
    extra = dict(seed=torch.tensor([987654321], dtype=torch.int64, device=DEV) if p > 0 else None, site=2, p=p)
    if nq:
        extra.update(lnw=1 + 0.1 * torch.randn(C, device=DEV), lnb=0.1 * torch.randn(C, device=DEV), wq=w(nq, C),
                     bq=0.1 * torch.randn(nq, device=DEV))
    a = _ext().sa_layer_fwd(qkv, x, N, 0.25, wo, bo, g2, be2, 1e-5, w1, b1, w2, b2, **extra)
    e = _emu().sa_layer_fwd(qkv, x, N, 0.25, wo, bo, g2, be2, 1e-5, w1, b1, w2, b2, **extra)
    names = ["o", "lse", "z", "y", "mean2", "rstd2", "u"] + (["next", "mean1", "rstd1"] if nq else [])
    assert len(a) == len(e) == len(names)
    errs = {n: rel_fro(u, v) for u, v, n in zip(a, e, names)}
    assert all(v < 1e-2 for v in errs.values()), errs
