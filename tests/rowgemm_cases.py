"""What the row-pass kernel variant tests share (a plain module, no fixtures): seeded operands of the
``csrc/rowgemm.hip`` entry points, misaligned copies of them, the host-side launch arithmetic the
tests steer by (``split_tiles``, ``pick_nch``, the slab-job block count) and a float64 autograd
evaluation of the layer-boundary composite.

Every operand is drawn on the CPU from one seeded generator and then moved, so the CPU and the GPU
tests see the same values.  Weights are bf16 (what the kernels read), everything else fp32 unless a
test narrows it.
"""
import math

import torch
import torch.nn.functional as F

EPS = 1e-5
BF = torch.bfloat16

PA_GRADS = ("dWo", "dbo", "dg2", "dbe2", "dW1", "db1", "dW2", "db2")
LL_GRADS = ("dlnw", "dlnb", "dW", "dbias")
BOUNDARY_NAMES = ("dy", "dO", "delta", "dlnw", "dlnb", "dWq", "dbq") + PA_GRADS


# ---- the launchers' host arithmetic (rowgemm.hip split_tiles / pick_nch, binding.cpp make_job) ----
def split_tiles(R):
    t = (R + 63) // 64
    return 4 if t <= 64 else 2 if t < 128 else 1


def pick_nch(K):
    n = (K + 31) // 32
    return n if n <= 2 else 4 if n <= 4 else 5 if n <= 5 else 8


def job_nblk(S, P, target=128, cols=1024):
    """workgroups of a non-deterministic slab job over an (S, P) slab"""
    nbx = (P + cols - 1) // cols
    nsy = max(1, min(S, target // nbx))
    rb = (S + nsy - 1) // nsy
    return nbx * ((S + rb - 1) // rb)


# ---- comparisons --------------------------------------------------------------------------------
def rel_fro(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def tile_rel_fro(a, b, rows=64):
    """the relative Frobenius error of every 64-row tile of a row output (leading axis = rows; the
    last tile may be partial), as a 1-D float64 tensor"""
    a, b = a.double().cpu(), b.double().cpu()
    R = a.shape[0]
    a, b = a.reshape(R, -1), b.reshape(R, -1)
    pad = (-R) % rows
    if pad:
        a = torch.cat([a, a.new_zeros(pad, a.shape[1])])
        b = torch.cat([b, b.new_zeros(pad, b.shape[1])])
    a, b = a.reshape(-1, rows * a.shape[1]), b.reshape(-1, rows * b.shape[1])
    return (a - b).norm(dim=1) / (b.norm(dim=1) + 1e-30)


# ---- operand placement --------------------------------------------------------------------------
def off1(t):
    """a contiguous copy of t that starts one element into a larger allocation: 2 bytes off a
    16-byte boundary for bf16, 4 bytes for fp32 (the launchers' av_ok then fails)"""
    if t is None:
        return None
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 != 0
    return v


def off1_all(d, keys=None):
    """d with the tensors under keys (default: every tensor) replaced by off1 copies"""
    return {k: off1(v) if torch.is_tensor(v) and (keys is None or k in keys) else v for k, v in d.items()}


def slab_layout(sizes):
    """(offsets, row length) of a slab row whose segments start at multiples of 4 floats"""
    offs, P = [], 0
    for n in sizes:
        offs.append(P)
        P += (n + 3) // 4 * 4
    return offs, P


def slab_views(tiles, sizes, device, fill=float("nan")):
    offs, P = slab_layout(sizes)
    slab = torch.full((tiles, P), fill, device=device)
    return slab, [slab[:, o:o + n] for o, n in zip(offs, sizes)], offs


def pa_sizes(C):
    return [C * C, C, C, C, C * C, C, C * C, C]


def pa_shapes(C):
    return [(C, C), (C,), (C,), (C,), (C, C), (C,), (C, C), (C,)]


# one slab job for every carrier: 8 segments, a partial last 1024-column block, 7 rows →
# 13 column blocks × 7 row splits = 91 workgroups, a multiple of neither 2 nor 4
JOB_ROWS, JOB_SIZES = 7, pa_sizes(64)


def make_job(device, seed=0):
    """(slab, destinations, offsets, initial destinations) of a slab-reduction job"""
    g = torch.Generator().manual_seed(4242 + seed)
    offs, P = slab_layout(JOB_SIZES)
    slab = torch.randn(JOB_ROWS, P, generator=g).to(device)
    init = [torch.randn(n, generator=g).to(device) for n in JOB_SIZES]
    return slab, [t.clone() for t in init], offs, init


def job_bound(slab, init, offs):
    """per destination element: the largest difference between two fp32 summations, in any order,
    of its S slab terms and its initial value — each is within S·2⁻²⁴·Σ|terms| of the exact sum"""
    S = slab.shape[0]
    mass = slab.abs().double().sum(0)
    return [(S * 2.0 ** -23) * (mass[o:o + t.numel()] + t.abs().double()) for t, o in zip(init, offs)]


# ---- operands -----------------------------------------------------------------------------------
def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) + 11)


def ln_linear_operands(R, Kin, N, device, seed=0):
    """x, w, the LN affine, bias and residual of ln_linear_fwd; g, dres and the row statistics of
    ln_linear_bwd / wgrad; u: a bf16 activation for wgrad's GELU mode"""
    g = _gen(R, Kin, N, seed)

    def rn(*s, sc=1.0):
        return torch.randn(*s, generator=g) * sc

    x = rn(R, Kin) * 1.5 + 0.3
    d = dict(x=x, w=(rn(N, Kin) / math.sqrt(Kin)).to(BF), lnw=1 + 0.3 * rn(Kin), lnb=0.3 * rn(Kin), bias=rn(N),
             res=rn(R, N), g=rn(R, N), dres=rn(R, Kin), mean=x.mean(-1),
             rstd=torch.rsqrt(x.var(-1, unbiased=False) + EPS), u=rn(R, Kin).to(BF))
    return {k: v.to(device) for k, v in d.items()}


def post_attn_operands(R, C, device, seed=0):
    """operands of post_attn_fwd / post_attn_ln_linear_fwd (o … bq) and the upstream gradient dz of
    post_attn_bwd; the scales are those of tests/test_kernels_gpu.py test_post_attn"""
    g = _gen(R, C, seed, 3)

    def rn(*s, sc=1.0):
        return torch.randn(*s, generator=g) * sc

    def w(*s):
        return (rn(*s) / math.sqrt(s[-1])).to(BF)

    d = dict(o=rn(R, C).to(BF), x=rn(R, C), wo=w(C, C), bo=0.1 * rn(C), g2=1 + 0.3 * rn(C), be2=0.3 * rn(C),
             w1=w(C, C), b1=0.1 * rn(C), w2=w(C, C), b2=0.1 * rn(C), lnw=1 + 0.3 * rn(C), lnb=0.3 * rn(C),
             wq=w(3 * C, C), bq=0.1 * rn(3 * C), dz=rn(R, C))
    return {k: v.to(device) for k, v in d.items()}


PA_FWD = ("o", "x", "wo", "bo", "g2", "be2", "w1", "b1", "w2", "b2")
NEXT = ("lnw", "lnb", "wq", "bq")


def pa_fwd_args(d):
    return [d[k] for k in PA_FWD[:6]] + [EPS] + [d[k] for k in PA_FWD[6:]]


def boundary_operands(R, C, nq, device, seed=0):
    """the operands of tests/test_kernels_gpu.py test_ln_linear_post_attn_bwd_isolated at any C:
    layer l+1's LN1 + in-projection backward (g, wq, x, its row statistics, dres) and layer l's
    post-attention backward (y, its statistics, u, o, the three weights, LN2's affine)"""
    gen = _gen(R, C, nq, seed, 5)

    def rn(*s, sc=1.0):
        return torch.randn(*s, generator=gen) * sc

    def w(*s):
        return rn(*s, sc=0.15).to(BF)

    x, y = rn(R, C), rn(R, C)
    d = dict(g=rn(R, nq), wq=w(nq, C), x=x, mean1=x.mean(1), rstd1=torch.rsqrt(x.var(1, unbiased=False) + EPS),
             lnw=1 + 0.1 * rn(C), lnb=0.1 * rn(C), dres=rn(R, C), y=y, m2=y.mean(1),
             r2=torch.rsqrt(y.var(1, unbiased=False) + EPS), u=rn(R, C).to(BF), o=rn(R, C).to(BF), wo=w(C, C), w1=w(C, C),
             w2=w(C, C), g2=1 + 0.1 * rn(C), be2=0.1 * rn(C))
    return {k: v.to(device) for k, v in d.items()}


def boundary_sizes(C, nq):
    return [C, C, nq * C, nq] + pa_sizes(C)


def run_boundary(K, d, H, targets, **kw):
    """K.ln_linear_post_attn_bwd over the operands d into the 12 slab views ``targets``"""
    return K.ln_linear_post_attn_bwd(d["g"], d["wq"], d["x"], d["mean1"], d["rstd1"], d["lnw"], d["lnb"], d["dres"],
                                     targets[:4], d["y"], d["m2"], d["r2"], d["u"], d["o"], d["wo"], d["w1"], d["w2"],
                                     d["g2"], d["be2"], H, targets[4:], **kw)


def slab_sums(slab, sizes):
    offs, _ = slab_layout(sizes)
    tot = slab.float().sum(0)
    return [tot[o:o + n] for o, n in zip(offs, sizes)]


# ---- the float64 composite of the layer boundary ------------------------------------------------
def _ln64(x, w, b):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + EPS) * w + b


def boundary_composite_fp64(d, g, dres, H):
    """float64 autograd of: out-projection, residual, LayerNorm, MLP with GELU, residual, then
    LayerNorm and linear — L = Σ qkv∘g + Σ z∘dres over post_attn_operands d.  Returns the 15 outputs
    of the boundary backward by name (BOUNDARY_NAMES)."""
    p = {k: d[k].detach().double().cpu().requires_grad_(True) for k in PA_FWD + NEXT}
    y = p["x"] + p["o"] @ p["wo"].t() + p["bo"]
    y.retain_grad()
    h = F.gelu(_ln64(y, p["g2"], p["be2"]) @ p["w1"].t() + p["b1"])
    z = y + h @ p["w2"].t() + p["b2"]
    qkv = _ln64(z, p["lnw"], p["lnb"]) @ p["wq"].t() + p["bq"]
    ((qkv * g.double().cpu()).sum() + (z * dres.double().cpu()).sum()).backward()
    R, C = y.shape
    do = p["o"].grad
    delta = (do.view(R, H, C // H) * p["o"].detach().view(R, H, C // H)).sum(-1)
    grads = [p[k].grad for k in ("lnw", "lnb", "wq", "bq", "wo", "bo", "g2", "be2", "w1", "b1", "w2", "b2")]
    return dict(zip(BOUNDARY_NAMES, [y.grad, do, delta] + grads))


def boundary_emulation(emu, d, g, dres, H):
    """the same 15 outputs from emulation.post_attn_fwd → emulation.ln_linear_post_attn_bwd"""
    z, y, m2, r2, u = emu.post_attn_fwd(*pa_fwd_args(d))
    _, mean1, rstd1 = emu.ln_linear_fwd(z, d["lnw"], d["lnb"], EPS, d["wq"], d["bq"], 0, None, True, True)
    R, C = y.shape
    sizes = boundary_sizes(C, 3 * C)
    slab, tg, _ = slab_views((R + 63) // 64, sizes, y.device, 0.0)
    b = dict(g=g, wq=d["wq"], x=z, mean1=mean1, rstd1=rstd1, lnw=d["lnw"], lnb=d["lnb"], dres=dres, y=y, m2=m2, r2=r2,
             u=u, o=d["o"], wo=d["wo"], w1=d["w1"], w2=d["w2"], g2=d["g2"], be2=d["be2"])
    outs = run_boundary(emu, b, H, tg)
    return dict(zip(BOUNDARY_NAMES, list(outs) + slab_sums(slab, sizes)))
