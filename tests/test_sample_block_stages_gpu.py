"""The optional stages of the per-sample block kernels (csrc/sample_block.hip ``sb_fwd`` / ``sb_bwd`` /
``sb_wgrad``) on the GPU, stage by stage, on the cases of tests/sample_block_cases.py:

* pre (a cross layer's post-attention half; per-sample and broadcast x_q), post with N = C (a query
  projection) and N = 2C (a decoder's K|V, the ``two`` branch), an empty ``dres``, ``zero_out``, the
  slab job of ``sb_wgrad`` (16 segments; a subset), uneven ``sb_wgrad`` row splits (R = 544) and the
  4-layer block the binding admits;
* every returned tensor against the fp32 emulation (ops/emulation.py) on the same operands with
  ``close`` at its default bounds (relative Frobenius ≤ 1 %, max-abs ≤ 2 % of the reference's
  largest value) and, per sample, the same 1 % relative Frobenius bound; the backward reads the
  kernel's own saved tensors on both sides, so bf16 rounding ties of the forward do not enter;
* two cases against the float64 composite at 2 % (per sample), so kernel and emulation cannot
  share a mistake;
* bitwise repeatability (no atomics in ``sb_fwd`` / ``sb_bwd``), the host refusals, and an image
  classifier's training step with the folds on and off through the real kernels.

No bound here departs from ``close``'s defaults."""
import pytest
import torch

import sample_block_cases as sbc

pytestmark = pytest.mark.gpu

DEV = "cuda"
SAMPLE_BOUND = 1e-2  # close's relative Frobenius bound, per sample
F64_BOUND = 2e-2     # tests/test_sample_block_gpu.py: kernel against the full-precision composite


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


def close_per_sample(a, b, B, name):
    """``close`` and the per-sample relative Frobenius bound of a tensor with a sample axis"""
    assert torch.isfinite(a).all(), name
    close(a, b, name=name)
    e = sbc.sample_rel_fro(a, b, B)
    print(f"{name}: worst sample rel fro {e:.3e}")
    assert e <= SAMPLE_BOUND, f"{name}: a sample's relative Frobenius error is {e:.3e}"


def _kernels():
    from perceiver_io_amd.ops import emulation, ext

    return ext.require(), emulation


@pytest.fixture(scope="module")
def runs():
    """per case, computed once: the operands; the kernels' and the emulation's forward; the kernels'
    and the emulation's backward, both over the KERNEL's forward outputs"""
    cache = {}

    def get(name):
        if name not in cache:
            K, emu = _kernels()
            c = sbc.case(name, DEV)
            xk, fk = sbc.run_fwd(K, c)
            xe, fe = sbc.run_fwd(emu, c)
            bk = sbc.run_bwd(K, c, xk, fk)
            be = sbc.run_bwd(emu, c, xk.clone(), fk)
            torch.cuda.synchronize()
            cache[name] = dict(c=c, xk=xk, fk=fk, xe=xe, fe=fe, bk=bk, be=be)
        return cache[name]

    return get


@pytest.mark.parametrize("name", list(sbc.CASES))
def test_forward_matches_emulation(name, runs):
    """all 12·L saved tensors, the pre stage's 6, the post stage's [Q, LN_q(z), mean, rstd], and x
    after the call (the pre stage's output; untouched without a pre stage)"""
    r = runs(name)
    c = r["c"]
    if c["pre"]:
        close_per_sample(r["xk"], r["xe"], c["B"], "x after the call")
    else:
        assert torch.equal(r["xk"], c["x"])
    got, want = sbc.named_fwd(c, r["fk"]), sbc.named_fwd(c, r["fe"])
    assert [n for n, _ in got] == [n for n, _ in want]
    for (n, a), (_, b) in zip(got, want):
        assert a.dtype == b.dtype, n
        close_per_sample(a, b, c["B"], n)


@pytest.mark.parametrize("name", list(sbc.CASES))
def test_backward_matches_emulation(name, runs):
    """dx, the LayerNorm slab column range by column range, per layer dQKV / dY / dU / dZ, the pre
    tail dO, δ, dY, dU, dZ and the post tail dQb"""
    r = runs(name)
    c = r["c"]
    assert r["bk"]["slab"].shape == r["be"]["slab"].shape == (c["B"], sbc.slab_width(c))
    got, want = sbc.named_bwd(c, r["bk"]), sbc.named_bwd(c, r["be"])
    assert [n for n, _ in got] == [n for n, _ in want]
    for (n, a), (_, b) in zip(got, want):
        assert a.dtype == b.dtype, n
        close_per_sample(a, b, c["B"], n)


@pytest.mark.parametrize("name", list(sbc.CASES))
def test_forward_and_backward_repeat_bitwise(name, runs):
    """sb_fwd and sb_bwd use no atomics: a second call returns the same bits in every output"""
    K, _ = _kernels()
    r = runs(name)
    c = r["c"]
    x2, f2 = sbc.run_fwd(K, c)
    assert torch.equal(x2, r["xk"])
    for (n, a), (_, b) in zip(sbc.named_fwd(c, f2), sbc.named_fwd(c, r["fk"])):
        assert torch.equal(a, b), n
    b2 = sbc.run_bwd(K, c, r["xk"], r["fk"])
    assert torch.equal(b2["slab"], r["bk"]["slab"])
    for (n, a), (_, b) in zip(sbc.named_bwd(c, b2), sbc.named_bwd(c, r["bk"])):
        assert torch.equal(a, b), n


def test_empty_dres_equals_zero_dres(runs):
    """post stage, empty dres (the kernel's ``dres == nullptr`` path): the same bits as a dres of zeros"""
    K, _ = _kernels()
    r = runs("B5_L3_C64_pre_bcast_post2C_empty_dres")
    c = r["c"]
    assert c["dres"].numel() == 0
    io = sbc.post_io(c, r["fk"])
    zeros = torch.zeros(c["R"], c["C"], device=DEV)
    bz = sbc.run_bwd(K, c, r["xk"], r["fk"], post_io=[io[0], zeros, io[2], io[3]])
    for (n, a), (_, b) in zip(sbc.named_bwd(c, r["bk"]), sbc.named_bwd(c, bz)):
        assert torch.equal(a, b), n


@pytest.mark.parametrize("name,n4", [
    ("B5_L3_C64_pre_bcast_post2C_empty_dres", 3),        # fewer float4 than workgroups
    ("B17_L2_C128_pre_alone_uneven_wgrad_splits", 1031),  # not a multiple of B = 17
    ("B5_L3_C64_pre_bcast_post2C_empty_dres", 35),       # an exact multiple of B = 5
    ("B17_L2_C128_pre_alone_uneven_wgrad_splits", 1020),  # an exact multiple of B = 17
])
def test_zero_out_clears_exactly_its_slice(name, n4, runs):
    """zero_out: every element of the slice is cleared, nothing before or after it is touched, and
    the backward's own outputs do not change"""
    K, _ = _kernels()
    r = runs(name)
    c = r["c"]
    pad = 64
    buf = torch.full((2 * pad + 4 * n4,), 7.0, device=DEV)
    view = buf[pad:pad + 4 * n4]
    assert view.data_ptr() % 16 == 0
    bz = sbc.run_bwd(K, c, r["xk"], r["fk"], zero_out=view)
    torch.cuda.synchronize()
    assert (buf[:pad] == 7.0).all() and (buf[pad + 4 * n4:] == 7.0).all()
    assert (view == 0).all(), (view != 0).nonzero().flatten()[:8]
    for (n, a), (_, b) in zip(sbc.named_bwd(c, bz), sbc.named_bwd(c, r["bk"])):
        assert torch.equal(a, b), n


def _guarded_targets(c, tg):
    """moves the slab destinations of ``tg`` into one flat buffer with 4 guard floats (7.0) after
    each → the buffer"""
    C = c["C"]
    segs = [n for n, _ in sbc.slab_segments(c)]
    flat = torch.full((len(segs) * (C + 4),), 7.0, device=DEV)
    for k, n in enumerate(segs):
        v = flat[k * (C + 4):k * (C + 4) + C]
        v.copy_(tg[n])
        tg[n] = v
    return flat


@pytest.mark.parametrize("name,skip", [(n, ()) for n in sbc.CASES] + [
    ("B5_L3_C128_pre_bcast_post2C_16_slab_segments_two_branch", ("L1.g2", "post.b"))],
    ids=list(sbc.CASES) + ["B5_L3_C128_slab_subset_two_destinations_left_out"])
def test_wgrad_with_slab_job_matches_emulation(name, skip, runs):
    """sb_wgrad with the slab job appended (jobs with N ∈ {C, 2C, 3C}; 16 segments, a subset of 14,
    fewer; R = 544 splits the rows 288 + 256): dW / db and the slab destinations start from non-zero
    values and are added to; destinations left out, and the guard floats between destinations, do
    not move"""
    K, emu = _kernels()
    r = runs(name)
    c = r["c"]
    C = c["C"]
    jobs = sbc.wgrad_jobs(c, r["fk"], r["bk"])
    if "16_slab_segments" in name:
        assert len(jobs) == 16 and len(sbc.slab_segments(c)) == 16
        assert {G.shape[1] for _, _, G, _ in jobs} == {C, 2 * C, 3 * C}
    init = sbc.wgrad_targets(c, jobs, fill=5)
    res = []
    for mod in (K, emu):
        tg = {n: t.clone() for n, t in init.items()}
        flat = _guarded_targets(c, tg)
        sbc.run_wgrad(mod, c, jobs, r["bk"]["slab"], tg, skip=skip)
        torch.cuda.synchronize()
        guards = flat.view(-1, C + 4)[:, C:]
        assert (guards == 7.0).all()
        res.append(tg)
    got, want = res
    for n in init:
        if n in skip:
            assert torch.equal(got[n], init[n]), n
            continue
        assert not torch.equal(got[n], init[n]), n
        close(got[n], want[n], name=n)
        close(got[n] - init[n], want[n] - init[n], name=n + " (increment)")


@pytest.mark.parametrize("name", sbc.F64_CASES)
def test_kernels_match_float64_composite(name, runs):
    """the kernels' forward, backward and weight gradients against float64 autograd of pre stage → L
    layers → post projection: 2 % relative Frobenius, per sample where there is a sample axis"""
    K, _ = _kernels()
    r = runs(name)
    c = r["c"]
    jobs = sbc.wgrad_jobs(c, r["fk"], r["bk"])
    tg = sbc.wgrad_targets(c, jobs)
    sbc.run_wgrad(K, c, jobs, r["bk"]["slab"], tg)
    torch.cuda.synchronize()
    ferr, berr = sbc.reference_errors(c, r["xk"], r["fk"], r["bk"], tg, sbc.reference(c))
    errs = {**ferr, **berr}
    for k, v in errs.items():
        print(f"{k}: {v:.3e}")
    bad = {k: v for k, v in errs.items() if not v < F64_BOUND}
    assert not bad, bad


# ---- host refusals: TORCH_CHECKs that fire before any launch ----

def _one_job(n=1):
    def rows():
        return torch.zeros(32, 64, device=DEV, dtype=torch.bfloat16)

    return [t for _ in range(n) for t in (rows(), rows(), torch.zeros(64, 64, device=DEV), torch.zeros(64, device=DEV))]


def test_refuses_20_jobs():
    K, _ = _kernels()
    with pytest.raises(RuntimeError, match="jobs"):
        K.sb_wgrad(_one_job(20))


def test_refuses_20_segment_slab():
    K, _ = _kernels()
    slab = torch.ones(2, 80, device=DEV)
    dsts = [torch.zeros(4, device=DEV) for _ in range(20)]
    jobs = _one_job()
    with pytest.raises(RuntimeError, match="16 segments"):
        K.sb_wgrad(jobs, job_slab=slab, job_dsts=dsts, job_offs=[4 * k for k in range(20)])
    torch.cuda.synchronize()
    assert all((d == 0).all() for d in dsts) and (jobs[2] == 0).all()


def test_refuses_x_q_of_64_rows_for_5_samples(runs):
    K, _ = _kernels()
    c = runs("B5_L3_C64_pre_bcast_post2C_empty_dres")["c"]
    pre = list(c["pre"])
    pre[1] = torch.zeros(64, c["C"], device=DEV)
    with pytest.raises(RuntimeError, match="x_q"):
        K.sb_fwd(c["x"].clone(), c["kp"], c["scale"], c["eps"], pre=pre, post=c["post"])


def test_refuses_post_weight_of_3C_rows(runs):
    K, _ = _kernels()
    c = runs("B5_L3_C64_pre_bcast_post2C_empty_dres")["c"]
    C = c["C"]
    post = [c["post"][0], c["post"][1], torch.zeros(3 * C, C, device=DEV, dtype=torch.bfloat16),
            torch.zeros(3 * C, device=DEV)]
    with pytest.raises(RuntimeError, match="C or 2C outputs"):
        K.sb_fwd(c["x"].clone(), c["kp"], c["scale"], c["eps"], pre=c["pre"], post=post)


# ---- model level: the folds on and off through the real kernels ----

@pytest.mark.parametrize("ch", [64, 128])
def test_classifier_step_with_folds_on_and_off(ch, monkeypatch):
    """tests/test_sample_block_pre.py on the GPU: an image classifier's loss and gradients with
    SB_PRE / SB_POST / SB_KV all on against all off (loss within 2e-3·max(1, |loss|), gradients
    within 1 % of the largest gradient) and against the eager ``torch`` backend (3 %); the folded run
    hands the kernels a pre stage, a query projection and a decoder's 2C-wide K|V, the unfolded run
    none; no hand-off is left behind"""
    from perceiver_io_amd import ops
    from perceiver_io_amd.ops import fused
    from test_sample_block_pre import _model

    torch.manual_seed(ch + 1)
    model = _model(ch, 3, 2).to(DEV)
    x = torch.randn(3, 28, 28, 1, device=DEV)
    y = torch.tensor([1, 7, 3], device=DEV)

    def grads():
        return {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}

    with ops.backend("torch"):
        torch.nn.functional.cross_entropy(model(x), y).backward()
    g_ref = grads()
    real = fused.kernels
    calls = []

    class Recording:  # the executor's kernel calls, sb_fwd's stage operands noted
        def __init__(self, K):
            self.K = K

        def __getattr__(self, name):
            fn = getattr(self.K, name)
            if name != "sb_fwd":
                return fn

            def sb_fwd(*a, pre=(), post=(), **kw):
                calls.append((len(pre), tuple(post[2].shape) if len(post) else None))
                return fn(*a, pre=pre, post=post, **kw)
            return sb_fwd

    monkeypatch.setattr(fused, "kernels", lambda t: Recording(real(t)))
    old = fused.SB_PRE, fused.SB_POST, fused.SB_KV
    res = []
    try:
        for fold in (False, True):
            fused.SB_PRE = fused.SB_POST = fused.SB_KV = fold
            calls.clear()
            model.zero_grad(set_to_none=True)
            loss = model.loss(x, y)
            loss.backward()
            torch.cuda.synchronize()
            res.append((loss.item(), grads(), list(calls)))
            for k in ("bwd_q", "have_q", "have_pa", "bwd_pa"):
                assert fused._LOOKAHEAD[k] is None, (fold, k)
    finally:
        fused.SB_PRE, fused.SB_POST, fused.SB_KV = old
    (l0, g0, c0), (l1, g1, c1) = res
    assert len(c0) == len(c1) == 3, (c0, c1)
    assert all(c == (0, None) for c in c0), c0
    assert [c[0] for c in c1] == [10, 10, 10], c1
    assert [c[1] for c in c1] == [(ch, ch), (ch, ch), (2 * ch, ch)], c1
    print(f"loss folded {l1:.6f} unfolded {l0:.6f}")
    assert abs(l1 - l0) < 2e-3 * max(1.0, abs(l0))
    assert set(g1) == set(g0) == set(g_ref)
    gmax = max(g.abs().max() for g in g_ref.values())
    for n in g0:
        assert (g1[n] - g0[n]).abs().max() < 0.01 * gmax, n
        assert (g1[n] - g_ref[n]).abs().max() < 0.03 * gmax, n
        assert (g0[n] - g_ref[n]).abs().max() < 0.03 * gmax, n
