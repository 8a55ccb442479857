"""Inputs and float64 references for the vocabulary cross-entropy heads (csrc/ce_head.hip at C = 64,
csrc/mlm_head.hip at C = 32 / 128) and for mlm_select (csrc/mlm_select.hip); shared by
tests/test_vocab_head_edges.py (CPU) and tests/test_vocab_head_edges_gpu.py.

Every builder draws on the CPU from a seeded generator, so a case is the same tensors wherever it is
moved.  ``h`` is bf16-exact fp32 and ``w`` bf16 (the kernels cast on load), ``bias`` fp32.

The reference is the definition in float64:
  logits = h·wᵀ + bias,  lse = logsumexp(logits),  loss = Σ_{label ≥ 0} (lse − logits[label]) / max(count, 1)
  dl = (softmax − onehot)·[label ≥ 0]·gout / max(count, 1),  dH = dl·w,  dW = dlᵀ·h,  db = Σ_rows dl
"""
import math
from types import SimpleNamespace

import torch

LOG2E = 1.4426950408889634
SHAPES_ALL_C = [(1, 1000), (127, 1000), (128, 1000), (129, 1000), (63, 300), (65, 300),
                (70, 65), (70, 96), (70, 97), (70, 127), (70, 129), (5, 200), (600, 1100)]
# (130, 256 | 257): the C = 64 backward's one-hot-in-tile instance on and off; (5, 4100): the shape the
# head's issue names for the forward's split cap — vocab_splits() gives 13 there, and 16 (the cap) at
# (5, 4090), so both are run
SHAPES_C64 = [(130, 256), (130, 257), (5, 4100), (5, 4090)]
FAMILY_SHAPES = [(130, 2003), (5, 4100), (5, 4090)]
RAMPS = ("ramp_up", "ramp_down", "ramp_slow", "ramp_sparse", "gathered")
FAMILIES = ("baseline", "ramp_up", "ramp_down", "ramp_slow", "ramp_sparse", "spike_last", "spike_split", "spike_label",
            "offset_neg", "offset_pos", "repeat", "count_gout", "gathered")


def shapes(C):
    return SHAPES_ALL_C + (SHAPES_C64 if C == 64 else [])


def family_cases(C):
    out = [(f, M, V) for f in FAMILIES for (M, V) in FAMILY_SHAPES if C == 64 or V != 4090]
    return out + [("repeat", 130, 200)]


def bf(x):
    return x.to(torch.bfloat16).float()


def specials(V):
    return [s for s in (0, V - 1, 63, 64, 127, 128) if s < V]


def vocab_splits(M, V, rows_per_wg=128, chunk=64, max_splits=16):
    """the forward's vocabulary split count at C = 64 (ce_head.hip vocab_splits)"""
    rb, nchunks = -(-M // rows_per_wg), -(-V // chunk)
    s = max(1, -(-512 // rb))
    s = min(s, (nchunks + 3) // 4, max_splits)
    cps = -(-nchunks // s)
    return -(-nchunks // cps)


def bwd_row_splits(C, M, V):
    """the slab height of ce_bwd(slab=True): ce2_bwd_splits (C = 64) / ce_dw_splits"""
    nt = -(-M // 64)
    if C == 64:
        vb = -(-V // 128)
        s = max(1, min(-(-512 // vb), (nt + 3) // 4))
    else:
        nch = -(-V // 64)
        s = max(1, min(-(-1024 // nch), nt))
    tps = -(-nt // s)
    return -(-nt // tps)


def make_case(family, C, M, V):
    fi = FAMILIES.index(family) if family in FAMILIES else len(FAMILIES)
    g = torch.Generator().manual_seed(100003 * C + 977 * M + V + 31 * fi)
    wscale = 0.05 if family in RAMPS else 0.3
    h = bf(torch.randn(M, C, generator=g))
    w = torch.randn(V, C, generator=g) * wscale
    bias = torch.randn(V, generator=g) * 0.1
    lab = torch.randint(0, V, (M,), generator=g)
    sp = specials(V)
    for i in range(min(M - 1, 2 * len(sp))):
        lab[1 + i] = sp[(i + 1) % len(sp)]
    v = torch.arange(V)
    blk = (v // 32).float()
    count, gout, idx = None, 0.37, None
    if family in ("ramp_up", "gathered"):
        bias = bias + 6.0 * blk
    elif family == "ramp_down":
        bias = bias - 6.0 * blk
    elif family == "ramp_slow":
        bias = bias + 5.0 * blk
    elif family == "ramp_sparse":
        # one riser per 32-entry block, 5.0 (7.2 log2 units) above the last one and 25 above its own
        # block, in alternating 16-entry halves: every other block is packed against a stale reference
        pos = (v // 32 % 2) * 4
        bias = bias + 5.0 * blk - 25.0 * (v % 32 != pos).float()
    elif family == "spike_last":
        bias[V - 1] += 60.0
    elif family == "spike_split":  # the spike in the first chunk (split 0), every label in the last 64 entries
        bias[5] += 60.0
        lab = V - 1 - torch.randint(0, min(64, V // 8), (M,), generator=g)
    elif family == "spike_label":
        # two rows of three: the row's own label 60 above the rest, through a channel of its own
        # (h = 8, w = 7.5, zero elsewhere); every third row is an ordinary one, so that the per-row
        # floor 1e-3·max_r ‖ref[r]‖ is set by real gradients and the ≈ 0 rows are held to it
        k = len(sp)
        w[:, :k] = 0.0
        h[:, :k] = 0.0
        for r in range(M):
            if r % 3:
                j = r % k
                lab[r] = sp[j]
                h[r, j] = 8.0
                w[sp[j], j] = 7.5
    elif family == "offset_neg":
        bias = bias - 300.0
    elif family == "offset_pos":
        bias = bias + 300.0
    elif family == "repeat":
        lab[:] = 777 if V > 1000 else 77
    elif family == "count_gout":
        count, gout = 57.0, -1.7
    lab[::7] = -100
    if family == "no_labels":
        lab[:] = -100
        count = 0.0
    if count is None:
        count = float((lab >= 0).sum())
    if family == "gathered":
        idx = torch.randperm(2 * M, generator=g)[:M]
        hbig = bf(torch.randn(2 * M, C, generator=g))
        hbig[idx] = h
        h = hbig
    rowmap = torch.randperm(3 * M, generator=g)[:M]
    return SimpleNamespace(name=f"{family}-C{C}-M{M}-V{V}", family=family, C=C, M=M, V=V, h=h.contiguous(), idx=idx,
                           labels=lab, w=w.to(torch.bfloat16).contiguous(), bias=bias.float().contiguous(),
                           count=torch.tensor([count]), gout=torch.tensor([gout]), rowmap=rowmap)


def to(case, dev):
    d = SimpleNamespace(**vars(case))
    for k, x in vars(case).items():
        if torch.is_tensor(x):
            setattr(d, k, x.to(dev))
    return d


def rows(d):
    return d.h if d.idx is None else d.h.index_select(0, d.idx)


# ---- float64 reference ----------------------------------------------------------------------------
def logits64(d):
    return bf(rows(d)).double() @ d.w.double().t() + d.bias.double()


def reference(d):
    h, w = bf(rows(d)).double(), d.w.double()
    logits = h @ w.t() + d.bias.double()
    lse = torch.logsumexp(logits, -1)
    valid = d.labels >= 0
    n = max(float(d.count.item()), 1.0)
    safe = d.labels.clamp(min=0)
    picked = logits.gather(1, safe[:, None])[:, 0]
    loss = torch.where(valid, lse - picked, torch.zeros_like(lse)).sum() / n
    onehot = torch.zeros_like(logits).scatter_(1, safe[:, None], 1.0)
    dl = (torch.exp(logits - lse[:, None]) - onehot) * valid[:, None].double() * (float(d.gout.item()) / n)
    dH = dl @ w
    dHmap = torch.zeros(3 * d.M, d.C, dtype=torch.float64, device=dH.device)
    dHmap.index_add_(0, d.rowmap[valid], dH[valid])
    return dict(lse=lse, loss=loss, dH=dH, dH_map=dHmap, dW=dl.t() @ h, db=dl.sum(0), logit_max=logits.abs().amax(1))


def ulp32(x):
    """spacing of fp32 numbers at |x| (float64 tensor)"""
    x = x.abs().clamp_min(2.0 ** -126)
    return torch.pow(2.0, torch.floor(torch.log2(x)) - 23)


def row_err(x, ref):
    """‖x[r] − ref[r]‖ / max(‖ref[r]‖, 1e-3·max_r ‖ref[r]‖) per row (per entry of a vector)"""
    x = x.double().reshape(ref.shape)
    if ref.dim() == 1:
        n, e = ref.abs(), (x - ref).abs()
    else:
        n, e = ref.norm(dim=1), (x - ref).norm(dim=1)
    return e / torch.maximum(n, 1e-3 * n.max()).clamp_min(1e-300)


def rel_fro(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


BWD_NAMES = ("dH", "dW", "db", "dH_map", "dW_acc", "db_acc", "dH_slab", "dW_slab", "db_slab")
REF_OF = dict(dH="dH", dW="dW", db="db", dH_map="dH_map", dW_acc="dW", db_acc="db", dH_slab="dH", dW_slab="dW",
              db_slab="db")


def backward_variants(K, d, hs, lse, ref, **u):
    """ce_bwd of ``K`` (the extension or the emulation) four ways: overwriting, accumulating into
    non-zero targets with a rowmap into a (3M, C) dH, and slab=True (slab rows summed, padding sliced
    off).  Accumulated outputs are returned minus their initial values, in float64."""
    M, V, C, dev = d.M, d.V, d.C, d.w.device
    g = torch.Generator().manual_seed(99)
    init = {n: (torch.randn(ref[n].shape, generator=g).to(dev) * float(ref[n].abs().max())).float()
            for n in ("dH_map", "dW", "db")}
    out = {}
    dH, dW, db = torch.zeros(M, C, device=dev), torch.full((V, C), 7.0, device=dev), torch.full((V,), -3.0, device=dev)
    K.ce_bwd(hs, d.labels, d.w, d.bias, lse, d.gout, d.count, dH, dW, db, False, None, **u)
    out.update(dH=dH, dW=dW, db=db)
    dH2, dW2, db2 = init["dH_map"].clone(), init["dW"].clone(), init["db"].clone()
    K.ce_bwd(hs, d.labels, d.w, d.bias, lse, d.gout, d.count, dH2, dW2, db2, True, d.rowmap, **u)
    out.update(dH_map=dH2.double() - init["dH_map"].double(), dW_acc=dW2.double() - init["dW"].double(),
               db_acc=db2.double() - init["db"].double())
    dH3 = torch.zeros(M, C, device=dev)
    sl = K.ce_bwd(hs, d.labels, d.w, d.bias, lse, d.gout, d.count, dH3, dW.clone(), db.clone(), False, None, slab=True, **u)
    tot = sl.double().sum(0)
    out.update(dH_slab=dH3, dW_slab=tot[:V * C].view(V, C), db_slab=tot[V * C:V * C + V], slab_rows=sl.shape[0],
               slab_cols=sl.shape[1])
    return out


# ---- the C = 64 forward's lazy reference max, replayed in float64 ---------------------------------
def rescale_trace(logits):
    """Per row, ce_head.hip's rule on the 32-entry blocks of the vocabulary: the reference max m_ref
    moves only on a re-base, and a block re-bases when Σ 2^(t·log2e − m_ref) over either 16-entry
    half (accumulator rows 8q + 4h + 0..3 of half h) exceeds 256.  → (rebased (M, nblk) bool, the
    largest p of each block against the reference it was packed with (M, nblk))."""
    M, V = logits.shape
    nblk = -(-V // 32)
    t = torch.full((M, nblk * 32), -math.inf, dtype=torch.float64)
    t[:, :V] = logits.double().cpu() * LOG2E
    t = t.view(M, nblk, 32)
    half = (torch.arange(32) // 4) % 2
    m_ref = torch.full((M,), -math.inf, dtype=torch.float64)
    rebased = torch.zeros(M, nblk, dtype=torch.bool)
    pmax = torch.zeros(M, nblk, dtype=torch.float64)
    for b in range(nblk):
        p = torch.pow(2.0, t[:, b] - m_ref[:, None])  # +inf against m_ref = −inf
        over = ~((p[:, half == 0].sum(1) <= 256.0) & (p[:, half == 1].sum(1) <= 256.0))
        m_ref = torch.where(over, torch.maximum(m_ref, t[:, b].amax(1)), m_ref)
        rebased[:, b] = over
        pmax[:, b] = torch.pow(2.0, t[:, b] - m_ref[:, None]).amax(1)
    return rebased, pmax


# ---- mlm_select ------------------------------------------------------------------------------------
def select_loop(labels, cap, gcap):
    """mlm_select as a plain loop over sequences and positions → idx_b, lab_b, gidx, glab, total, overflow"""
    B, L = labels.shape
    lab = labels.tolist()
    idx_b = [[j % L for j in range(cap)] for _ in range(B)]
    lab_b = [[-100] * cap for _ in range(B)]
    gidx, glab = [0] * gcap, [-100] * gcap
    total = used = 0
    over = False
    for b in range(B):
        n = 0
        for i in range(L):
            if lab[b][i] != -100:
                if n < cap:
                    idx_b[b][n], lab_b[b][n] = i, lab[b][i]
                    if used < gcap:
                        gidx[used], glab[used] = b * cap + n, lab[b][i]
                    used += 1
                n += 1
        total += n
        over = over or n > cap
    over = over or used > gcap
    return (torch.tensor(idx_b), torch.tensor(lab_b), torch.tensor(gidx), torch.tensor(glab),
            torch.tensor([float(total)]), torch.tensor([over]))


def _planted(B, L, counts, gen):
    """labels (B, L) with exactly counts[b] selected positions in sequence b, at random places"""
    lab = torch.full((B, L), -100, dtype=torch.int64)
    for b, n in enumerate(counts):
        at = torch.randperm(L, generator=gen)[:n]
        lab[b, at] = torch.randint(3, 1000, (n,), generator=gen)
    return lab


def _random(B, L, p, gen):
    lab = torch.randint(3, 1000, (B, L), generator=gen)
    lab[torch.rand(B, L, generator=gen) > p] = -100
    return lab


def select_cases():
    """name → (labels, cap, gcap, overflow expected)"""
    g = torch.Generator().manual_seed(4242)
    c = {}
    a = _random(2, 1025, 0.15, g)
    a[0] = -100
    a[0, 1024] = 17   # sequence 0: every selected position in the second pass
    a[1, 1024] = -100  # sequence 1: none there
    c["two_passes"] = (a, 200, 400, False)
    a = _random(3, 2500, 0.12, g)
    a[0, :2048] = -100  # only in the third (partial) pass
    a[1, 2048:] = -100  # none in the third pass
    c["three_passes"] = (a, 300, 900, None)
    c["wide_batch"] = (_random(300, 40, 0.15, g), 8, 2400, None)
    c["all_selected"] = (torch.randint(3, 1000, (1, 64), generator=g), 64, 64, False)
    c["none_selected"] = (torch.full((4, 100), -100, dtype=torch.int64), 16, 32, False)
    c["count_eq_cap"] = (_planted(3, 50, [10, 3, 10], g), 10, 40, False)
    c["count_cap_plus_1"] = (_planted(3, 50, [10, 11, 3], g), 10, 40, True)
    c["used_eq_gcap"] = (_planted(3, 50, [10, 7, 3], g), 10, 20, False)
    c["used_gcap_plus_1"] = (_planted(3, 50, [10, 7, 4], g), 10, 20, True)
    return c


SELECT_NAMES = ("idx_b", "lab_b", "gidx", "glab", "total", "overflow")
