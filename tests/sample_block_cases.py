"""What the per-sample block stage tests share (a plain module, no fixtures): seeded operands of
``sb_fwd`` / ``sb_bwd`` / ``sb_wgrad`` (csrc/sample_block.hip, ops/emulation.py) with their optional
stages, the layout of what those calls return, and a float64 autograd evaluation of the whole
composite: pre stage (a cross layer's post-attention half) → L self-attention layers → post
projection (the next cross layer's LN + query projection, N = C, or a decoder's packed K|V, N = 2C).

Every operand is drawn on the CPU from one seeded generator and then moved, so the CPU and the GPU
tests see the same values.  O and x differ from sample to sample (an indexing fault changes
values); a broadcast x_q is one (32, C) tensor.
"""
import math

import torch

N, H = 32, 4
EPS = 1e-5

# (B, L, C, pre, post, dres): pre ∈ {None, "rows" (per-sample x_q), "bcast" ((32, C) x_q)},
# post = outputs of the post projection in units of C (0: none), dres ∈ {"given", "empty", None}
CASES = {
    "B1_L1_C64_pre_rows_postC_all_stages_one_workgroup": (1, 1, 64, "rows", 1, "given"),
    "B5_L3_C128_pre_bcast_post2C_16_slab_segments_two_branch": (5, 3, 128, "bcast", 2, "given"),
    "B5_L3_C64_pre_bcast_post2C_empty_dres": (5, 3, 64, "bcast", 2, "empty"),
    "B17_L2_C128_pre_alone_uneven_wgrad_splits": (17, 2, 128, "rows", 0, None),
    "B17_L2_C64_post_alone_postC_slab_offset": (17, 2, 64, None, 1, "given"),
    "B3_L4_C128_four_layers": (3, 4, 128, None, 0, None),
}
# the two cases also held against the float64 composite on the GPU (rows 2 and 4 of the table)
F64_CASES = ("B5_L3_C128_pre_bcast_post2C_16_slab_segments_two_branch", "B17_L2_C128_pre_alone_uneven_wgrad_splits")

LAYER_NAMES = ("g1", "be1", "wqkv", "bqkv", "wo", "bo", "g2", "be2", "w1", "b1", "w2", "b2")
PRE_NAMES = ("wo", "bo", "g2", "be2", "w1", "b1", "w2", "b2")
POST_NAMES = ("g", "b", "w", "bias")
SAVED_NAMES = ("ln1x", "qkv", "o", "ln2y", "u", "gu", "y", "z", "mean1", "rstd1", "mean2", "rstd2")
PRE_SAVED_NAMES = ("ln2y", "u", "gu", "y", "mean2", "rstd2")
POST_SAVED_NAMES = ("q", "lnx", "mean", "rstd")


def rel_fro(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def sample_rel_fro(a, b, B):
    """the largest per-sample relative Frobenius error of a tensor whose leading axis holds B
    samples (B·32 rows, or B slab rows)"""
    a, b = a.double().cpu().reshape(B, -1), b.double().cpu().reshape(B, -1)
    return ((a - b).norm(dim=1) / (b.norm(dim=1) + 1e-30)).max().item()


def make_case(B, L, C, pre, post, dres, device, seed=0):
    """Operands of one case on ``device``.  Weights are bf16 (what the kernels read), everything else
    fp32; the scales are those of tests/test_sample_block_gpu.py ``_params``."""
    g = torch.Generator().manual_seed(1000 * seed + 97 * B + 13 * L + C)
    R = B * N
    bf = torch.bfloat16

    def rn(*s, sc=1.0):
        return torch.randn(*s, generator=g) * sc

    def lin(n_out):  # a bf16 (n_out, C) weight and its fp32 bias
        return rn(n_out, C, sc=0.08).to(bf), rn(n_out, sc=0.05)

    def to(ts):
        return [t.to(device).contiguous() for t in ts]

    kp = []
    for _ in range(L):
        wqkv, bqkv = lin(3 * C)
        g1, be1 = 1 + rn(C, sc=0.1), rn(C, sc=0.1)
        wo, bo = lin(C)
        g2, be2 = 1 + rn(C, sc=0.1), rn(C, sc=0.1)
        w1, b1 = lin(C)
        w2, b2 = lin(C)
        kp += [g1, be1, wqkv, bqkv, wo, bo, g2, be2, w1, b1, w2, b2]
    case = dict(B=B, L=L, C=C, R=R, scale=1.0 / math.sqrt(C // H), eps=EPS, kp=to(kp), pre=[], post=[], dq=None,
                dres=None, pre_kind=pre, post_n=post * C, dres_kind=dres)
    if pre:
        o = rn(R, C).to(bf)
        xq = rn(R if pre == "rows" else N, C)
        wo, bo = lin(C)
        g2, be2 = 1 + rn(C, sc=0.1), rn(C, sc=0.1)
        w1, b1 = lin(C)
        w2, b2 = lin(C)
        case["pre"] = to([o, xq, wo, bo, g2, be2, w1, b1, w2, b2])
        # the block input is the pre stage's output: the forward writes it, nothing may read it first
        case["x"] = torch.full((R, C), float("nan"), device=device)
    else:
        case["x"] = rn(R, C).to(device)
    case["dz"] = rn(R, C).to(device)
    if post:
        w, bias = lin(post * C)
        case["post"] = to([1 + rn(C, sc=0.1), rn(C, sc=0.1), w, bias])
        case["dq"] = rn(R, post * C).to(device)
        dr = rn(R, C)
        case["dres"] = dr.to(device) if dres == "given" else torch.empty(0, device=device)
    return case


def case(name, device, seed=0):
    return make_case(*CASES[name], device=device, seed=seed)


def post_io(c, fwd):
    """sb_bwd's post_io of a case from a forward's outputs"""
    return [c["dq"], c["dres"], fwd["post"][2], fwd["post"][3]] if c["post"] else []


def split_fwd(c, out):
    """sb_fwd's list → {"saved": 12·L, "pre": 6 or [], "post": [Q, LN_q(z), mean, rstd] or []}"""
    L = c["L"]
    want = 12 * L + (6 if c["pre"] else 0) + (4 if c["post"] else 0)
    assert len(out) == want, (len(out), want)
    k = 12 * L + (6 if c["pre"] else 0)
    return dict(saved=list(out[:12 * L]), pre=list(out[12 * L:k]), post=list(out[k:]))


def split_bwd(c, out):
    """sb_bwd's list → {"dx", "slab", "layers": L × [dQKV, dY, dU, dZ], "pre": [dO, δ, dY, dU, dZ]
    or [], "post": [dQb] or []}"""
    L = c["L"]
    want = 2 + 4 * L + (5 if c["pre"] else 0) + (1 if c["post"] else 0)
    assert len(out) == want, (len(out), want)
    k = 2 + 4 * L
    return dict(dx=out[0], slab=out[1], layers=[list(out[2 + 4 * i:6 + 4 * i]) for i in range(L)],
                pre=list(out[k:k + 5]) if c["pre"] else [], post=[out[-1]] if c["post"] else [])


def named_fwd(c, fwd):
    """(name, tensor) of every tensor a forward returned"""
    out = [(f"L{i}.{n}", fwd["saved"][12 * i + j]) for i in range(c["L"]) for j, n in enumerate(SAVED_NAMES)]
    out += [(f"pre.{n}", t) for n, t in zip(PRE_SAVED_NAMES, fwd["pre"])]
    out += [(f"post.{n}", t) for n, t in zip(POST_SAVED_NAMES, fwd["post"])]
    return out


def named_bwd(c, bwd):
    """(name, tensor) of every tensor a backward returned, the slab column range by column range"""
    C = c["C"]
    out = [("dx", bwd["dx"])]
    out += [(f"slab.{n}", bwd["slab"][:, o:o + C]) for n, o in slab_segments(c)]
    for i, lay in enumerate(bwd["layers"]):
        out += [(f"L{i}.{n}", t) for n, t in zip(("dqkv", "dy", "du", "dz"), lay)]
    out += [(f"pre.{n}", t) for n, t in zip(("do", "delta", "dy", "du", "dz"), bwd["pre"])]
    out += [(f"post.{n}", t) for n, t in zip(("dqb",), bwd["post"])]
    return out


def slab_width(c):
    return (4 * c["L"] + (2 if c["pre"] else 0) + (2 if c["post"] else 0)) * c["C"]


def slab_segments(c):
    """(gradient name, first column) of every C-wide segment of the LayerNorm partial slab: per
    layer dγ1 | dβ1 | dγ2 | dβ2, then the pre stage's dγ2 | dβ2, then the post stage's dγ | dβ"""
    L, C = c["L"], c["C"]
    segs = [(f"L{i}.{n}", (4 * i + j) * C) for i in range(L) for j, n in enumerate(("g1", "be1", "g2", "be2"))]
    o = 4 * L * C
    if c["pre"]:
        segs += [("pre.g2", o), ("pre.be2", o + C)]
        o += 2 * C
    if c["post"]:
        segs += [("post.g", o), ("post.b", o + C)]
    return segs


def wgrad_jobs(c, fwd, bwd):
    """[(weight name, bias name, G, A)] of the block's weight gradients, in the order ops/fused.py
    queues them: per layer (dQKV, LN1(x)), (dY, O), (dU, LN2(y)), (dZ, GELU(u)); the post stage's
    (dQb, LN_q(z)); the pre stage's (dY, O), (dU, LN2(y)), (dZ, GELU(u))"""
    jobs = []
    for i in range(c["L"]):
        dq, dy, du, dzz = bwd["layers"][i]
        sv = fwd["saved"][12 * i:12 * (i + 1)]
        jobs += [(f"L{i}.wqkv", f"L{i}.bqkv", dq, sv[0]), (f"L{i}.wo", f"L{i}.bo", dy, sv[2]),
                 (f"L{i}.w1", f"L{i}.b1", du, sv[3]), (f"L{i}.w2", f"L{i}.b2", dzz, sv[5])]
    if c["post"]:
        jobs.append(("post.w", "post.bias", bwd["post"][0], fwd["post"][1]))
    if c["pre"]:
        _, _, dy, du, dzz = bwd["pre"]
        jobs += [("pre.wo", "pre.bo", dy, c["pre"][0]), ("pre.w1", "pre.b1", du, fwd["pre"][0]),
                 ("pre.w2", "pre.b2", dzz, fwd["pre"][2])]
    return jobs


def run_fwd(K, c):
    """``K.sb_fwd`` on a fresh clone of the case's x (the forward writes it with a pre stage) →
    (the block input after the call, split_fwd's dict)"""
    x = c["x"].clone()
    out = K.sb_fwd(x, c["kp"], c["scale"], c["eps"], pre=c["pre"], post=c["post"])
    return x, split_fwd(c, out)


def run_bwd(K, c, x0, fwd, **kw):
    """``K.sb_bwd`` of the case over a forward's outputs (kw: zero_out, or another post_io)"""
    if c["pre"]:
        kw.update(pre=c["pre"], pre_saved=fwd["pre"])
    if c["post"]:
        kw.setdefault("post_io", post_io(c, fwd))
        kw.update(post=c["post"])
    return split_bwd(c, K.sb_bwd(c["dz"], x0, fwd["saved"], c["kp"], c["scale"], c["eps"], **kw))


def wgrad_targets(c, jobs, fill=None):
    """{name: fp32 target} of every weight / bias gradient of ``jobs`` and every slab segment:
    zeros, or seeded non-zero values (fill = a seed; the kernels add)"""
    dev, C = c["x"].device, c["C"]
    g = None if fill is None else torch.Generator().manual_seed(fill)
    shapes = {}
    for wn, bn, G, A in jobs:
        shapes[wn], shapes[bn] = (G.shape[1], C), (G.shape[1],)
    for n, _ in slab_segments(c):
        shapes[n] = (C,)
    return {n: (torch.zeros(s) if g is None else torch.randn(s, generator=g)).to(dev) for n, s in shapes.items()}


def run_wgrad(K, c, jobs, slab, tg, skip=()):
    """``K.sb_wgrad`` of ``jobs`` with the slab reduction into the targets ``tg`` (slab segments named
    in ``skip`` are left out, as ops/fused.py leaves out a frozen parameter's)"""
    flat = [t for wn, bn, G, A in jobs for t in (G, A, tg[wn], tg[bn])]
    segs = [(n, o) for n, o in slab_segments(c) if n not in skip]
    K.sb_wgrad(flat, job_slab=slab, job_dsts=[tg[n] for n, _ in segs], job_offs=[o for _, o in segs])


def reference_errors(c, x0, fwd, bwd, tg, ref):
    """({forward output: error}, {gradient: error}) of one forward / backward / weight-gradient
    pass against ``reference(c)``: relative Frobenius errors, the largest per-sample one for every
    tensor with a sample axis — the block input after the call (the pre stage's output), the block
    output, Q; dx, dO, δ; the reduced LayerNorm slab segments and every dW / db (``tg``)"""
    B, L = c["B"], c["L"]
    z = fwd["saved"][12 * (L - 1) + 7]
    ferr = {"x0": sample_rel_fro(x0, ref["x0"], B), "z": sample_rel_fro(z, ref["z"], B)}
    if c["post"]:
        assert fwd["post"][0].shape == (c["R"], c["post_n"])
        ferr["q"] = sample_rel_fro(fwd["post"][0], ref["q"], B)
    assert bwd["slab"].shape == (B, slab_width(c))
    berr = {"dx": sample_rel_fro(bwd["dx"], ref["dx"], B)}
    if c["pre"]:
        assert bwd["pre"][1].shape == (c["R"], H)
        berr["do"] = sample_rel_fro(bwd["pre"][0], ref["do"], B)
        berr["delta"] = sample_rel_fro(bwd["pre"][1], ref["delta"], B)
    assert set(tg) == set(ref["grads"]), set(tg) ^ set(ref["grads"])
    for n, t in tg.items():
        berr[n] = rel_fro(t, ref["grads"][n].view(t.shape))
    return ferr, berr


def _ln(x, g, b):
    return torch.nn.functional.layer_norm(x, (x.shape[-1],), g, b, EPS)


def _half(y, p):
    """z = y + MLP(LN2(y)) with p = {g2, be2, w1, b1, w2, b2}"""
    u = _ln(y, p["g2"], p["be2"]) @ p["w1"].t() + p["b1"]
    return y + torch.nn.functional.gelu(u) @ p["w2"].t() + p["b2"]


def reference(c):
    """float64 autograd of the composite on the CPU.  Returns {"x0": the block input (the pre
    stage's output when there is one), "z": the block output, "q": the post projection or None,
    "dx": gradient of the block's residual input rows (x_q's rows with a pre stage — per row, also
    for a broadcast x_q —, x's otherwise), "do": gradient of O or None, "delta": rowsum(dO∘O) per
    head (R, 4) or None, "grads": {name: gradient} of every parameter, named as slab_segments /
    wgrad_jobs name them}.  The loss is Σ z·dz without a post stage, Σ z·dres + Σ Q·dQ with one."""
    B, L, C, R = c["B"], c["L"], c["C"], c["R"]
    d = C // H

    def leaf(t):
        return t.detach().double().cpu().requires_grad_()

    layers = [dict(zip(LAYER_NAMES, (leaf(t) for t in c["kp"][12 * i:12 * (i + 1)]))) for i in range(L)]
    params = {f"L{i}.{n}": t for i, p in enumerate(layers) for n, t in p.items()}
    o_in = None
    if c["pre"]:
        o_in = leaf(c["pre"][0])
        xq = c["pre"][1]
        res = leaf(xq if xq.shape[0] == R else xq.repeat(B, 1))  # a row's own gradient either way
        pp = dict(zip(PRE_NAMES, (leaf(t) for t in c["pre"][2:])))
        params.update({f"pre.{n}": t for n, t in pp.items()})
        x = _half(o_in @ pp["wo"].t() + pp["bo"] + res, pp)
    else:
        res = leaf(c["x"])
        x = res
    x0 = x
    x = x.view(B, N, C)
    for p in layers:
        qkv = _ln(x, p["g1"], p["be1"]) @ p["wqkv"].t() + p["bqkv"]
        q, k, v = (t.reshape(B, N, H, d).transpose(1, 2) for t in qkv.split(C, -1))
        a = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(d), -1)
        o = (a @ v).transpose(1, 2).reshape(B, N, C)
        x = _half(x + o @ p["wo"].t() + p["bo"], p)
    z = x.reshape(R, C)
    qout = None
    if c["post"]:
        qp = dict(zip(POST_NAMES, (leaf(t) for t in c["post"])))
        params.update({f"post.{n}": t for n, t in qp.items()})
        qout = _ln(z, qp["g"], qp["b"]) @ qp["w"].t() + qp["bias"]
        loss = (qout * c["dq"].double().cpu()).sum()
        if c["dres"] is not None and c["dres"].numel():
            loss = loss + (z * c["dres"].double().cpu()).sum()
    else:
        loss = (z * c["dz"].double().cpu()).sum()
    loss.backward()
    out = dict(x0=x0.detach(), z=z.detach(), q=None if qout is None else qout.detach(), dx=res.grad, do=None,
               delta=None, grads={n: t.grad for n, t in params.items()})
    if o_in is not None:
        out["do"] = o_in.grad
        out["delta"] = (o_in.grad * o_in.detach()).view(R, H, d).sum(-1)
    return out
